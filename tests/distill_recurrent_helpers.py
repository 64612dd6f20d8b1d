"""The one copy of what the recurrent-distillation tests share (tests/test_distill_recurrent.py on the CPU, tests/test_gpu_distill_recurrent.py on
the GPU):
  - `np_update`: a numpy fp64 restatement of `RecurrentDistillation.update` written out by hand - forward, the cell's backward formulas, the
    explicit cuts (a done, a group boundary, an epoch's first step), clip and Adam; no autograd.  `defect=` plants one wrong rule.
  - `walk_update`: the same update as a split-and-pad walk through `nn.LSTM` itself: every env's steps of a group are cut into pieces at the
    dones and at an epoch's first step, each piece one `nn.LSTM` call from zeros, from (h0, c0) or from the explicitly detached carried state.
  - the shapes, the done pattern, the cases and the torch rule's references in fp64 / fp32, computed once and read-only.
`torch` is imported inside the functions: the module imports wherever its users do."""
import copy
import functools
import types

import numpy as np

import bptt_helpers as bh

# T, N, H, obs, head, A, gradient length, epochs: the smallest shapes at which tile edges (128 x 128), slice edges (16) and the group logic can go wrong
SHAPES = {
    "one": dict(T=1, N=1, H=1, obs=1, head=(1,), A=1, gl=1, epochs=1),
    "ragged": dict(T=5, N=134, H=20, obs=45, head=(32, 16), A=12, gl=3, epochs=2),            # a group wraps the epoch boundary, one step is left over
    "long-group": dict(T=2, N=134, H=20, obs=45, head=(32, 16), A=12, gl=5, epochs=3),         # one group over two epoch boundaries
    "4H-crosses-128": dict(T=4, N=133, H=132, obs=45, head=(128, 64), A=12, gl=3, epochs=2),
    "real-widths": dict(T=3, N=128, H=256, obs=45, head=(128, 128, 128), A=12, gl=2, epochs=3),
}
# the CPU tier of the rule: 6 envs
RULE_SHAPES = {
    "wrap+left-over": dict(T=5, N=6, H=7, obs=5, head=(8, 6), A=3, gl=3, epochs=2),
    "two-boundaries": dict(T=2, N=6, H=7, obs=5, head=(8, 6), A=3, gl=5, epochs=3),
    "gl-1": dict(T=5, N=6, H=7, obs=5, head=(8, 6), A=3, gl=1, epochs=2),
    "one-group": dict(T=5, N=6, H=7, obs=5, head=(8, 6), A=3, gl=10, epochs=2),
}
ALL_SHAPES = {**SHAPES, **RULE_SHAPES}
LEARNING_RATE = 1e-3
DEFECTS = ("gradient-crosses-a-done", "gradient-crosses-a-group-boundary", "gradient-crosses-an-epoch-boundary", "epoch-does-not-restart-from-h0",
           "carried-state-recomputed-after-the-step", "reset-one-step-late", "left-over-steps-back-propagated", "one-bias-without-gradient")
LSTM_NAMES = bh.LSTM_NAMES


def done_pattern(T, N):
    """`bptt_helpers.done_pattern` with the envs in two halves: a done at t = 0, two consecutive dones, a step where every row of the upper half is
    done, rows with none (in the lower half), dones at T - 1, which must not matter"""
    return bh.done_pattern(T, N, 2 if N >= 2 else 1)


def update_groups(s):
    from robot_lab_amd.distill import update_groups as ug

    return ug(s["T"], s["gl"], s["epochs"])


def make_policy(name, seed=3, teacher_recurrent=True):
    import torch

    from robot_lab_amd.distill_recurrent import StudentTeacherRecurrent

    s = ALL_SHAPES[name]
    torch.manual_seed(seed)
    return StudentTeacherRecurrent(s["obs"], s["obs"], s["A"], s["head"], (8,), init_noise_std=0.1, rnn_hidden_dim=s["H"], teacher_recurrent=teacher_recurrent)


def trained_named(pol):
    """[(state-dict name, parameter)] in the order of `trained_parameters()`"""
    out = [(f"memory_s.{k}", p) for k, p in pol.memory_s.named_parameters()] + [(f"student.{k}", p) for k, p in pol.student.named_parameters()]
    assert [id(p) for _, p in out] == [id(p) for p in pol.trained_parameters()]
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, seed, huber=False):
    """(StudentTeacherRecurrent on the host in fp32, {field: numpy array}) of the shape `name`, read-only.  `huber`: the teacher actions are wide
    enough that, in fp64 at the initial parameters, at least 10 % of d = student - teacher lie on either side of |d| = 1 (the Huber loss and its
    gradient are continuous there: no margin is needed)."""
    s = ALL_SHAPES[name]
    T, N, H, A = s["T"], s["N"], s["H"], s["A"]
    pol = make_policy(name)
    rng = np.random.default_rng(seed)
    f = dict(observations=rng.standard_normal((T, N, s["obs"])), teacher_actions=(1.5 if huber else 0.5) * rng.standard_normal((T, N, A)),
             h0=0.5 * rng.standard_normal((N, H)), c0=0.5 * rng.standard_normal((N, H)))
    f = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in f.items()}
    f["dones"] = done_pattern(T, N)
    for v in f.values():
        v.setflags(write=False)
    if huber and T * N * A >= 64:
        import torch

        p64 = copy.deepcopy(pol).double()
        with torch.no_grad():
            mean, _ = group_forward(p64, as_batch(f, torch.float64), list(range(T)), None)
        inside = float((np.abs(mean.numpy() - f["teacher_actions"]) < 1.0).mean())
        assert 0.1 <= inside <= 0.9, inside
    return pol, f


def as_batch(fields, dtype, device="cpu"):
    import torch

    fl = lambda a: torch.as_tensor(np.array(a)).to(device=device, dtype=dtype).contiguous()  # noqa: E731
    return types.SimpleNamespace(observations=fl(fields["observations"]), teacher_actions=fl(fields["teacher_actions"]), h0=fl(fields["h0"]), c0=fl(fields["c0"]),
                                 dones=torch.as_tensor(np.array(fields["dones"])).to(device))


def hyper(name, **kw):
    s = ALL_SHAPES[name]
    return {**dict(num_learning_epochs=s["epochs"], gradient_length=s["gl"], learning_rate=LEARNING_RATE), **kw}


def torch_alg(pol, dtype, name, device="cpu", **kw):
    from robot_lab_amd.distill_recurrent import RecurrentDistillation

    return RecurrentDistillation(copy.deepcopy(pol).to(device=device, dtype=dtype), **hyper(name, **kw))


def group_forward(pol, batch, steps, state):
    """(means [g, N, A], (h, c) behind the last step) of the epoch-relative steps `steps` in the rule's order from `state` (before the first step's
    reset; not read when steps[0] == 0), no gradient"""
    import torch

    from robot_lab_amd.distill_recurrent import lstm_step

    dones = batch.dones.to(torch.bool)
    h, c = state if state is not None else (None, None)
    means = []
    with torch.no_grad():
        for t in steps:
            if t == 0:
                h, c = batch.h0, batch.c0
            else:
                gone = dones[t - 1].unsqueeze(-1)
                h, c = torch.where(gone, torch.zeros_like(h), h), torch.where(gone, torch.zeros_like(c), c)
            h, c = lstm_step(pol.memory_s.rnn, batch.observations[t], h, c)
            means.append(pol.student(h))
    return torch.stack(means), (h, c)


def torch_group(pol, batch, steps, state, loss_type="mse"):
    """({name: gradient}, means, output state) of ONE group by torch autograd: the rule's loop body over `steps` from `state` as a value"""
    import torch

    from robot_lab_amd.distill import behavior_loss
    from robot_lab_amd.distill_recurrent import lstm_step

    loss_fn = behavior_loss(loss_type)
    dones = batch.dones.to(torch.bool)
    h, c = (state[0].detach(), state[1].detach()) if state is not None else (None, None)
    loss, means = 0, []
    for p in pol.trained_parameters():
        p.grad = None
    for t in steps:
        if t == 0:
            h, c = batch.h0.detach(), batch.c0.detach()
        else:
            gone = dones[t - 1].unsqueeze(-1)
            h, c = torch.where(gone, torch.zeros_like(h), h), torch.where(gone, torch.zeros_like(c), c)
        h, c = lstm_step(pol.memory_s.rnn, batch.observations[t], h, c)
        mean = pol.student(h)
        means.append(mean.detach())
        loss = loss + loss_fn(mean, batch.teacher_actions[t])
    loss.backward()
    g = {k: p.grad.detach().double().numpy().copy() for k, p in trained_named(pol)}
    return g, torch.stack(means).double().numpy(), (h.detach(), c.detach())


def recorded_update(alg, batch, name):
    """`alg.update(batch)` of a torch RecurrentDistillation with every group looked at: per group the parameters it ran on, the state it continued
    from, its means and output state and its gradient; then the result, the parameters, the Adam moments and the final state."""
    import torch

    s = ALL_SHAPES[name]
    groups, left = update_groups(s)
    pol = alg.policy
    rec = dict(groups=[])
    state = [None]

    def look(g):
        params = {k: p.detach().clone() for k, p in trained_named(pol)}
        means, out = group_forward(pol, batch, groups[g], state[0])
        grads = {k: p.grad.detach().double().numpy().copy() for k, p in trained_named(pol)}
        rec["groups"].append(dict(steps=groups[g], params=params, state_in=state[0], means=means.double().numpy(), state_out=out, grads=grads))
        state[0] = out

    alg.on_backward = look
    try:
        rec["result"] = alg.update(batch)
    finally:
        alg.on_backward = None
    assert len(rec["groups"]) == len(groups)
    if left:
        _, state[0] = group_forward(pol, batch, left, state[0])
    for a, b in zip(state[0], alg.final_state):  # the helper's forward is the rule's
        assert torch.allclose(a, b, rtol=1e-5 if a.dtype == torch.float32 else 1e-12, atol=0), float((a - b).abs().max())
    rec["params"] = {k: p.detach().double().numpy().copy() for k, p in trained_named(pol)}
    for what in ("exp_avg", "exp_avg_sq"):
        rec[what] = {k: alg.optimizer.state[p][what].detach().double().numpy().copy() for k, p in trained_named(pol)} if groups else {}
    rec["final_state"] = dict(h=alg.final_state[0].double().numpy(), c=alg.final_state[1].double().numpy())
    rec["step"] = len(groups)
    return rec


@functools.lru_cache(maxsize=None)
def _reference(name, seed, loss_type="mse", max_grad_norm=None):
    """{"f64" | "f32": recorded_update of the torch rule on the CPU}; in "f32" every group also carries `grads_at64` / `means_at64`: the fp32 rule's
    gradient and means of that group on the fp64 run's parameters and input state rounded to fp32 - what the device is handed.  "f32r" / "f32b":
    parameters, moments and final state of the fp32 rule on the same batch by two other fp32 routes - the envs in REVERSE order (another summation
    order), and the cell evaluated by nn.LSTM's own kernel instead of the written-out gates (other roundings inside the cell)."""
    import torch

    pol, f = build_case(name, seed, loss_type == "huber")
    out = {}
    for key, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        alg = torch_alg(pol, dtype, name, loss_type=loss_type, max_grad_norm=max_grad_norm)
        out[key] = recorded_update(alg, as_batch(f, dtype), name)
    b32 = as_batch(f, torch.float32)
    p32 = copy.deepcopy(pol)
    for g64, g32 in zip(out["f64"]["groups"], out["f32"]["groups"]):
        with torch.no_grad():
            for k, p in trained_named(p32):
                p.copy_(g64["params"][k].float())
        st = None if g64["state_in"] is None else tuple(t.float() for t in g64["state_in"])
        g32["grads_at64"], g32["means_at64"], so = torch_group(p32, b32, g64["steps"], st, loss_type)
        g32["state_out_at64"] = dict(h=so[0].double().numpy(), c=so[1].double().numpy())
    rev = {k: np.ascontiguousarray(v[:, ::-1] if k in ("observations", "teacher_actions", "dones") else v[::-1]) for k, v in f.items()}
    for key, fields, route in (("f32r", rev, None), ("f32b", f, _lstm_step_through_the_module)):
        alg = torch_alg(pol, torch.float32, name, loss_type=loss_type, max_grad_norm=max_grad_norm)
        import robot_lab_amd.distill_recurrent as dr

        written_out = dr.lstm_step
        try:
            dr.lstm_step = route or written_out
            alg.update(as_batch(fields, torch.float32))
        finally:
            dr.lstm_step = written_out
        back = (lambda a: a[::-1]) if key == "f32r" else (lambda a: a)
        out[key] = dict(params={k: p.detach().double().numpy() for k, p in trained_named(alg.policy)},
                        final_state=dict(h=back(alg.final_state[0].double().numpy()), c=back(alg.final_state[1].double().numpy())))
        for what in ("exp_avg", "exp_avg_sq"):
            out[key][what] = {k: alg.optimizer.state[p][what].detach().double().numpy() for k, p in trained_named(alg.policy)}
    return out


def _lstm_step_through_the_module(rnn, x, h, c):
    """the cell of `distill_recurrent.lstm_step` evaluated by nn.LSTM's own kernel: the same numbers by another fp32 route"""
    _, (hn, cn) = rnn(x.unsqueeze(0), (h.unsqueeze(0), c.unsqueeze(0)))
    return hn[0], cn[0]


YARDSTICK_FLOOR = bh.YARDSTICK_FLOOR
UPDATE_TENSORS = ("params", "exp_avg", "exp_avg_sq", "final_state")


def yardstick_measures(r):
    """Whether the YARDSTICK means something on a case, for every tensor the GPU tier bounds; a condition on the torch references alone (the learner
    under test is not consulted).  d is the fp32 torch rule's own distance from the fp64 torch rule, relative to max|ref64|.
      - Every group's means and gradient tensors, the Adam moments and the final state: d is at least half an fp32 spacing (2^-25), as
        `bptt_helpers.case_seed` asks - or the fp32 rule is exact (d < 1e-12: a saturated Huber row hands a bias the gradient 1 / (N A) exactly), and
        then the bound asks the device for the exact value too.  Where the fp32 reference merely happens to round well (a one-element tensor often
        does), e <= 8 d would ask for correctly rounded results, which no fp32 evaluation promises.  (Not asked of the parameters: after a step far
        below their spacing, a parameter's d is the rounding of the stored value itself, which seeds do not move.)
      - Parameters, moments and final state of the fp32 torch rule by two other fp32 routes - the envs in reverse order, and the cell through
        nn.LSTM's own kernel - lie within 8 d themselves.  Adam divides by sqrt(v) + 1e-8: where an entry's gradient is of the order of 1e-8 the step
        is lr g / 1e-8, round-off in g is amplified 1e5 times, and whether the fp32 rule's d shows it depends on its summation order; and a
        one-element tensor at the end of a chain of a dozen fp32 roundings lands anywhere within a few spacings.  A case on which the SAME rule by
        another fp32 route misses 8 d has a d that came out small by luck, and bounds nothing.
      - After ONE optimiser step a one-element exp_avg_sq is 0.001 g^2 where exp_avg is 0.1 g: to first order the square carries twice the relative
        error of g.  Where the fp32 rule's exp_avg_sq is CLOSER than its exp_avg, its roundings cancelled, and that d is no yardstick either."""
    def measured(v64, v32):
        scale = float(np.abs(v64).max())
        if not scale > 0:
            return False
        d = float(np.abs(np.asarray(v32) - np.asarray(v64)).max()) / scale
        return d >= YARDSTICK_FLOOR or d < 1e-12

    pairs = []
    for g64, g32 in zip(r["f64"]["groups"], r["f32"]["groups"]):
        pairs += [(g64["means"], g32["means_at64"])] + [(v, g32["grads_at64"][k]) for k, v in g64["grads"].items()]
    for what in UPDATE_TENSORS[1:]:
        pairs += [(r["f64"][what][k], r["f32"][what][k]) for k in r["f64"][what]]
    if not all(measured(a, b) for a, b in pairs):
        return False
    if r["f64"]["step"] == 1:  # (one optimiser step: exp_avg = 0.1 g, exp_avg_sq = 0.001 g^2, entry by entry)
        for k, v64 in r["f64"]["exp_avg"].items():
            if v64.size == 1:
                rel = lambda what: abs(float(r["f32"][what][k].reshape(-1)[0] - r["f64"][what][k].reshape(-1)[0]) / float(r["f64"][what][k].reshape(-1)[0]))  # noqa: E731
                if rel("exp_avg_sq") < rel("exp_avg"):
                    return False
    for what in UPDATE_TENSORS:
        for k, v64 in r["f64"][what].items():
            scale = float(np.abs(v64).max())
            d = float(np.abs(r["f32"][what][k] - v64).max()) / scale
            if not all(float(np.abs(r[route][what][k] - v64).max()) / scale <= 8.0 * d for route in ("f32r", "f32b")):
                return False
    return True


@functools.lru_cache(maxsize=None)
def case_seed(name, loss_type="mse", max_grad_norm=None):
    """The seed of the case (shape, loss type, clip): the first of 11, 12, ... 138 on which `yardstick_measures`."""
    for seed in range(11, 139):
        if yardstick_measures(_reference(name, seed, loss_type, max_grad_norm)):
            return seed
    raise AssertionError(f"{name} {loss_type} {max_grad_norm}: no seed in 11..138 gives a batch on which the fp32 reference measures every tensor")


def case(name, loss_type="mse", max_grad_norm=None):
    return build_case(name, case_seed(name, loss_type, max_grad_norm), loss_type == "huber")


def reference(name, loss_type="mse", max_grad_norm=None):
    return _reference(name, case_seed(name, loss_type, max_grad_norm), loss_type, max_grad_norm)


def split_flat(flat, pol):
    """{trained parameter name: its slice of a flat buffer in `trained_parameters()` order, fp64 on the host}"""
    out, o = {}, 0
    flat = flat.detach().double().cpu().numpy()
    for k, p in trained_named(pol):
        out[k] = flat[o:o + p.numel()].reshape(tuple(p.shape))
        o += p.numel()
    assert o == flat.size
    return out


within_bound = bh.within_bound


# ---- the numpy restatement ---------------------------------------------------------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def np_update(P, B, s, learning_rate=LEARNING_RATE, max_grad_norm=None, loss_type="mse", defect=None):
    """`RecurrentDistillation.update` in numpy fp64, no autograd.  P: {trained parameter name: array}; B: observations, teacher_actions, dones, h0,
    c0; s: T, gl, epochs.  Returns dict(groups=[{name: gradient}], params, final_state=dict(h, c), behavior)."""
    assert defect is None or defect in DEFECTS
    T, gl, epochs = s["T"], s["gl"], s["epochs"]
    f = lambda a: np.array(a, dtype=np.float64)  # noqa: E731
    p = {k: f(v) for k, v in P.items()}
    X, TA, dones, h0, c0 = f(B["observations"]), f(B["teacher_actions"]), np.asarray(B["dones"], dtype=bool), f(B["h0"]), f(B["c0"])
    N, A = TA.shape[1], TA.shape[2]
    L = len([k for k in p if k.startswith("student.") and k.endswith(".weight")])
    pre = "memory_s.rnn."
    m1, m2 = {k: np.zeros_like(v) for k, v in p.items()}, {k: np.zeros_like(v) for k, v in p.items()}
    seq = [(e, t) for e in range(epochs) for t in range(T)]
    full = len(seq) // gl
    chunks = [seq[i * gl:(i + 1) * gl] for i in range(full)] + ([seq[full * gl:]] if len(seq) % gl else [])

    def forward(par, chunk, h, c):
        recs = []
        H = par[pre + "weight_hh_l0"].shape[1]
        for e, t in chunk:
            restart = t == 0 and (e == 0 or defect != "epoch-does-not-restart-from-h0")
            if restart:
                h_in, c_in, keep, linked = h0, c0, np.ones((N, 1)), False
            else:
                tr = (t - 1) % T - (1 if defect == "reset-one-step-late" else 0)
                keep = (~dones[tr] if tr >= 0 else np.ones(N, dtype=bool))[:, None].astype(np.float64)
                h_in, c_in, linked = np.where(keep > 0, h, 0.0), np.where(keep > 0, c, 0.0), True
            z = X[t] @ par[pre + "weight_ih_l0"].T + par[pre + "bias_ih_l0"] + h_in @ par[pre + "weight_hh_l0"].T + par[pre + "bias_hh_l0"]
            i, fg, g, o = _sigmoid(z[:, :H]), _sigmoid(z[:, H:2 * H]), np.tanh(z[:, 2 * H:3 * H]), _sigmoid(z[:, 3 * H:])
            c = fg * c_in + i * g
            tc = np.tanh(c)
            h = o * tc
            recs.append(dict(t=t, x=X[t], h_in=h_in, c_in=c_in, keep=keep, linked=linked, i=i, f=fg, g=g, o=o, tc=tc, h=h, Whh=par[pre + "weight_hh_l0"]))
        return recs, h, c

    def head(par, recs):
        a = [np.concatenate([r["h"] for r in recs], 0)]
        for l in range(L):
            z = a[-1] @ par[f"student.{2 * l}.weight"].T + par[f"student.{2 * l}.bias"]
            a.append(np.where(z > 0, z, np.expm1(np.minimum(z, 0))) if l + 1 < L else z)
        d = a[-1] - np.concatenate([TA[r["t"]] for r in recs], 0)
        if loss_type == "mse":
            per, dmean = d * d, 2.0 * d
        else:
            ad = np.abs(d)
            per, dmean = np.where(ad <= 1.0, 0.5 * d * d, ad - 0.5), np.where(ad <= 1.0, d, np.sign(d))
        losses = [float(per[j * N:(j + 1) * N].mean()) for j in range(len(recs))]
        return a, dmean / (N * A), losses

    def backward(par, recs, before, a, dmean):
        grads = {}
        dz = dmean
        for l in range(L - 1, -1, -1):
            grads[f"student.{2 * l}.weight"] = dz.T @ a[l]
            grads[f"student.{2 * l}.bias"] = dz.sum(0)
            da = dz @ par[f"student.{2 * l}.weight"]
            dz = da * np.where(a[l] > 0, 1.0, a[l] + 1.0) if l > 0 else da  # elu' from the stored output; none behind the memory's output
        H = recs[0]["h"].shape[1]
        allr = before + recs
        dH = [np.zeros((N, H))] * len(before) + [dz[j * N:(j + 1) * N] for j in range(len(recs))]
        dWih, dWhh, db = np.zeros_like(par[pre + "weight_ih_l0"]), np.zeros_like(par[pre + "weight_hh_l0"]), np.zeros(4 * H)
        dz_next = dc_next = None
        for j in range(len(allr) - 1, -1, -1):
            r = allr[j]
            dh, dc = dH[j].copy(), np.zeros((N, H))
            if j + 1 < len(allr):
                nx = allr[j + 1]
                flows = nx["linked"] or defect == "gradient-crosses-an-epoch-boundary"
                if flows:
                    kn = 1.0 if defect == "gradient-crosses-a-done" or not nx["linked"] else nx["keep"]
                    dh = dh + kn * (dz_next @ nx["Whh"])
                    dc = dc + kn * nx["f"] * dc_next
            dc = dc + dh * r["o"] * (1.0 - r["tc"] ** 2)
            dzt = np.concatenate([dc * r["g"] * r["i"] * (1.0 - r["i"]), dc * r["c_in"] * r["f"] * (1.0 - r["f"]), dc * r["i"] * (1.0 - r["g"] ** 2),
                                  dh * r["tc"] * r["o"] * (1.0 - r["o"])], 1)
            dWih += dzt.T @ r["x"]
            dWhh += dzt.T @ r["h_in"]
            db += dzt.sum(0)
            dz_next, dc_next = dzt, dc
        grads[pre + "weight_ih_l0"], grads[pre + "weight_hh_l0"], grads[pre + "bias_ih_l0"] = dWih, dWhh, db
        grads[pre + "bias_hh_l0"] = np.zeros_like(db) if defect == "one-bias-without-gradient" else db.copy()
        return grads

    out = dict(groups=[])
    h = c = None
    before, total, cnt, step = [], 0.0, 0, 0
    for chunk in chunks:
        h_start, c_start = h, c
        recs, h, c = forward(p, chunk, h, c)
        a, dmean, losses = head(p, recs)
        total += sum(losses)
        cnt += len(losses)
        if len(chunk) < gl and defect != "left-over-steps-back-propagated":
            break
        grads = backward(p, recs, before if defect == "gradient-crosses-a-group-boundary" else [], a, dmean)
        out["groups"].append(grads)
        norm = np.sqrt(sum(float((v ** 2).sum()) for v in grads.values()))
        coef = min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm else 1.0
        step += 1
        for k in p:
            g = grads[k] * coef
            m1[k] = m1[k] + 0.1 * (g - m1[k])
            m2[k] = m2[k] * 0.999 + 0.001 * g * g
            p[k] = p[k] - (learning_rate / (1.0 - 0.9 ** step)) * (m1[k] / (np.sqrt(m2[k]) / np.sqrt(1.0 - 0.999 ** step) + 1e-8))
        before = recs
        if defect == "carried-state-recomputed-after-the-step":
            _, h, c = forward(p, chunk, h_start, c_start)
    out.update(params=p, final_state=dict(h=h, c=c), behavior=total / cnt)
    return out


# ---- the walk through nn.LSTM ------------------------------------------------------------------------------------------------------------
def walk_update(pol, batch, s, learning_rate=LEARNING_RATE, max_grad_norm=None):
    """The update on an fp64 copy of `pol` with `nn.LSTM` itself and torch.optim.Adam: per group and env the steps are cut into pieces - at a
    step behind a done (from zeros), at an epoch's first step (from h0 / c0) and at the group's first step (from the carried state, explicitly
    detached) -, each piece ONE call of the module over its whole length (MSE loss).  Returns what `np_update` returns."""
    import torch

    pol = copy.deepcopy(pol).double()
    rnn = pol.memory_s.rnn
    opt = torch.optim.Adam(pol.trained_parameters(), lr=learning_rate)
    obs, ta, dones = batch.observations.double(), batch.teacher_actions.double(), batch.dones.to(torch.bool)
    T, N = obs.shape[0], obs.shape[1]
    groups, left = update_groups(s)
    out = dict(groups=[])
    carried = None  # per env (h, c), detached
    total, cnt = 0.0, 0
    for steps in list(groups) + ([left] if left else []):
        hs = [[None] * N for _ in steps]
        last = []
        for r in range(N):
            pieces, start = [], 0
            for j in range(1, len(steps) + 1):
                if j == len(steps) or steps[j] == 0 or bool(dones[steps[j] - 1, r]):
                    pieces.append((start, j))
                    start = j
            for lo, hi in pieces:
                t0 = steps[lo]
                if t0 == 0:
                    init = (batch.h0[r].double().detach(), batch.c0[r].double().detach())
                elif bool(dones[t0 - 1, r]):
                    init = (torch.zeros(rnn.hidden_size, dtype=torch.float64),) * 2
                else:
                    assert lo == 0
                    init = (carried[r][0].detach(), carried[r][1].detach())
                x = torch.stack([obs[steps[j], r] for j in range(lo, hi)]).unsqueeze(1)  # [len, 1, D]
                y, (hn, cn) = rnn(x, (init[0].reshape(1, 1, -1), init[1].reshape(1, 1, -1)))
                for j in range(lo, hi):
                    hs[j][r] = y[j - lo, 0]
            last.append((hn.reshape(-1), cn.reshape(-1)))
        loss = 0
        for j, t in enumerate(steps):
            l_t = torch.nn.functional.mse_loss(pol.student(torch.stack(hs[j])), ta[t])
            loss = loss + l_t
            total += float(l_t.detach())
            cnt += 1
        carried = [(h.detach(), c.detach()) for h, c in last]
        if len(steps) == s["gl"]:
            opt.zero_grad()
            loss.backward()
            out["groups"].append({k: p.grad.detach().numpy().copy() for k, p in trained_named(pol)})
            if max_grad_norm:
                torch.nn.utils.clip_grad_norm_(pol.trained_parameters(), max_grad_norm)
            opt.step()
    out.update(params={k: p.detach().numpy().copy() for k, p in trained_named(pol)},
               final_state=dict(h=torch.stack([h for h, _ in carried]).numpy(), c=torch.stack([c for _, c in carried]).numpy()), behavior=total / cnt)
    return out


def worst(got, ref):
    """the largest max|got - ref| / max|ref| over every group's gradient tensors, the final state and the final parameters"""
    w = 0.0
    pairs = [(a, b) for ga, gb in zip(got["groups"], ref["groups"]) for a, b in ((ga[k], gb[k]) for k in gb)]
    pairs += [(got["final_state"][k], ref["final_state"][k]) for k in ("h", "c")] + [(got["params"][k], ref["params"][k]) for k in ref["params"]]
    for a, b in pairs:
        w = max(w, float(np.abs(np.asarray(a) - np.asarray(b)).max()) / float(np.abs(np.asarray(b)).max()))
    return w

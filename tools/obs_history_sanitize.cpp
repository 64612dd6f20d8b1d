// obs_history_sanitize.cpp - a stand-alone host program that drives the observation-history path of the C-ABI (include/rl_env.h
// rl_env_set_obs_history) on the CPU lane emulator's sources under AddressSanitizer + UBSan: create, set history (mixed per-term
// lengths on both groups), reset, steps with time-out resets among them, a partial reset, the refusals, destroy - and checks the
// history rows against the frames it saw.  Host code only; it needs no device and is not part of any test tier.
//
//   python -c "import ctypes, sys; sys.path.insert(0, '.'); from robot_lab_amd.scene import load_bundle; \
//              d, _ = load_bundle('RobotLab-Isaac-Velocity-Flat-Unitree-A1-v0'); \
//              open('/tmp/a1_flat.desc', 'wb').write(ctypes.string_at(ctypes.addressof(d), ctypes.sizeof(d)))"
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -DRL_EMU_ONLY=31 \
//       -o /tmp/obs_history_sanitize tools/obs_history_sanitize.cpp          (31: the A1 instance, one lane per limb - seconds of g++)
//   /tmp/obs_history_sanitize /tmp/a1_flat.desc
#include "../tests/emu/rl_env_emu.cpp"

#include <cstdio>

static int die(const char* what) {
  std::fprintf(stderr, "FAILED: %s: %s\n", what, rl_env_last_error());
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: %s <raw rl_env_desc file>\n", argv[0]); return 2; }
  std::vector<char> raw(sizeof(rl_env_desc));
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(raw.data(), 1, raw.size(), f) != raw.size() || std::fgetc(f) != EOF) { std::fprintf(stderr, "%s is not a raw rl_env_desc of %zu bytes\n", argv[1], raw.size()); return 2; }
  std::fclose(f);
  const rl_env_desc* desc = reinterpret_cast<const rl_env_desc*>(raw.data());
  const int N = 16;
  std::vector<float> origins(3 * N, 0.f);
  for (int e = 0; e < N; ++e) { origins[3 * e] = 2.5f * (float)(e % 4); origins[3 * e + 1] = 2.5f * (float)(e / 4); }
  setenv("RL_EMU_SUB", "1", 1);
  rl_env* env = nullptr;
  if (rl_env_create(desc, nullptr, nullptr, origins.data(), N, 5, 0, &env)) return die("create");
  const int np = desc->task.n_policy, nc = desc->task.n_critic;
  std::vector<int32_t> hp(np), hc(nc, 2);
  for (int i = 0; i < np; ++i) hp[i] = (i * 3 + 3) % 4;  // 3 2 1 0 3 2 ...
  hc[nc - 1] = RL_MAX_OBS_HISTORY;
  std::vector<int32_t> bad(np, RL_MAX_OBS_HISTORY + 1);
  if (rl_env_set_obs_history(env, 0, bad.data(), np) == 0 || rl_env_set_obs_history(env, 0, hp.data(), np + 1) == 0 || rl_env_set_obs_history(env, 3, hp.data(), np) == 0)
    return die("a call that must be refused was accepted");
  if (rl_env_set_obs_history(env, 0, hp.data(), np) || rl_env_set_obs_history(env, 1, hc.data(), nc)) return die("set_obs_history");
  if (rl_env_set_obs_history(env, 0, hp.data(), np) == 0) return die("second call accepted");
  std::vector<int32_t> back(np);
  if (rl_env_obs_history(env, 0, back.data(), np) != np || back != hp) return die("rl_env_obs_history");
  int64_t shape[3]; int32_t nd, es; void* p;
  if (rl_env_reset(env, nullptr, 0, nullptr)) return die("reset");
  if (rl_env_get_buffer(env, RL_BUF_EPISODE_LENGTH, &p, shape, &nd, &es)) return die("buffer");
  static_cast<int64_t*>(p)[3] = rl_env_max_episode_length(env) - 2;
  std::vector<float> action((size_t)N * rl_env_num_actions(env), 0.f);
  const int hd = rl_env_obs_dim(env, 0);
  std::vector<float> prev;
  for (int step = 0; step < 6; ++step) {
    if (rl_env_get_buffer(env, RL_BUF_OBS_POLICY, &p, shape, &nd, &es)) return die("buffer");
    prev.assign(static_cast<float*>(p), static_cast<float*>(p) + (size_t)N * hd);
    if (step == 3) {
      const int32_t ids[2] = {1, N - 1};
      if (rl_env_reset(env, ids, 2, nullptr)) return die("partial reset");
    } else if (rl_env_step(env, action.data(), nullptr)) return die("step");
    void *row, *frame;
    if (rl_env_get_buffer(env, RL_BUF_OBS_POLICY, &row, shape, &nd, &es) || shape[1] != hd) return die("buffer");
    if (rl_env_get_buffer(env, RL_BUF_OBS_POLICY_FRAME, &frame, shape, &nd, &es)) return die("buffer");
    const int fd = (int)shape[1];
    // term 0 (3 wide, H = 3) of env 0, which nothing resets: [slot0 | slot1 | slot2] = [prev slot1 | prev slot2 | frame]
    const float *r = static_cast<float*>(row), *fr = static_cast<float*>(frame);
    for (int j = 0; j < 3; ++j)
      if (r[j] != prev[3 + j] || r[3 + j] != prev[6 + j] || r[6 + j] != fr[j]) { std::fprintf(stderr, "FAILED: step %d: history row of env 0 does not shift\n", step); return 1; }
    (void)fd;
  }
  if (rl_env_set_obs_history(env, 1, hc.data(), nc) == 0) return die("call after the first step accepted");
  if (rl_env_destroy(env)) return die("destroy");
  std::printf("ok: observation history on %d envs, policy row %d columns, 6 launches, refusals refused\n", N, hd);
  return 0;
}

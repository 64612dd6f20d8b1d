// rl_env_sub.inl - launcher of the env kernels of ONE lane mapping (RL_ENV_TU_SUB = 1: a lane per limb, 2: a lane pair per limb, 8: eight lanes per limb):
// compiled as a translation unit of its own (rl_env_sub1.hip / rl_env_sub2.hip / rl_env_sub8.hip) so that hipcc works on the mappings in parallel,
// or included by rl_env.hip under -DRL_ENV_SINGLE_TU.  Returns a hipError_t, or -2 when the build does not carry the instance.
#define RL_SUB_CAT2(a, b) a##b
#define RL_SUB_CAT(a, b) RL_SUB_CAT2(a, b)
extern "C" __attribute__((visibility("hidden"))) int RL_SUB_CAT(rl_env_launch_sub, RL_ENV_TU_SUB)(const void* cfg, const void* S, const void* T, int inst, size_t lds1, void* stream) {
  return launch_inst<RL_ENV_TU_SUB>(*static_cast<const LaunchCfg*>(cfg), *static_cast<const rl::KState*>(S), T, inst, lds1, (hipStream_t)stream);
}

// rollout_policy_kernel<Tbl, W, true> (mt_rollout_actor_critic): its 18 instantiations and their launch.  A translation unit
// of its own so that it compiles beside engine.hip, not behind it (manytor_amd/build.py): together they are the largest
// kernel family of the library.  The host side of the call is engine.hip's.
#include <hip/hip_runtime.h>

#include "engine_internal.h"
#include "kernels.h"
#include "table_dispatch.h"

namespace mt {

// The dynamic LDS of a launch: the tape kernel's target tile, and with a critic the lanes' x columns, [IN][kBlock], behind it.
size_t actor_critic_lds(const mt_engine* h, int n_in, bool critic) {
  return ((size_t)3 * h->K + (critic ? (size_t)n_in : 0)) * kBlock * sizeof(float);
}
// W holds the widest hidden layer of either network
template <class Tbl, int W>
static void launch_actor_critic_t(mt_handle h, const StepArgs& a, const ActorCriticArgs& r) {
  const size_t lds = actor_critic_lds(h, r.n_in[0], r.CL != 0);
  if (lds > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rollout_policy_kernel<Tbl, W, true>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL((rollout_policy_kernel<Tbl, W, true>), grid_for(a.n), dim3(kBlock), lds, h->stream, a, r);
}
void launch_actor_critic(mt_handle h, const StepArgs& a, const ActorCriticArgs& r, int width) {
  with_table(h, [&](auto tag) {
    using Tbl = typename decltype(tag)::type;
    if (width <= 32) return launch_actor_critic_t<Tbl, 32>(h, a, r);
    launch_actor_critic_t<Tbl, 64>(h, a, r);
  });
}

}  // namespace mt

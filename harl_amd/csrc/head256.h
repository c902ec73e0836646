// head256.h -- launchers of the 33..64-output action head on a 256-wide head input (head256.hip), called by dispatch_actor
// and harl_actor_head_fvp (heads.hip).  ActorArgs and FvpArgs live in an unnamed namespace (heads_common.h), so an argument
// block crosses the translation units as a pointer to its bytes: both sides include the same definition.
#pragma once
#include "common.h"

namespace harl {
// `actor_args`: the caller's ActorArgs, filled as for every other actor head kernel (act_dim in [33, 64], dw_part = NULL;
// Gaussian training: part_ls set).  The caller checks the launch (check_launch).
void launch_head256(const void *actor_args, bool discrete, bool train, int grid, hipStream_t s);
// Head part of HATRPO's Fisher-vector product for a Categorical head of 33..64 actions (k_head256_fvp).  `fvp_args`: the
// caller's FvpArgs (heads_common.h), filled as for k_actor_head_fvp.  The caller checks the launch.
void launch_head256_fvp(const void *fvp_args, int grid, hipStream_t s);
}  // namespace harl

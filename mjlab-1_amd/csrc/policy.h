// Host entry of csrc/policy.hip for the C ABI (capi.cpp: mjx_policy_act).  Host-only: no
// step kernel includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/mjx355.h"

namespace mjx {
// Validates the descriptor against the kernel's limits and enqueues the one launch on
// `stream`.  Returns 0, or -1 with *err set and nothing launched.
__attribute__((visibility("hidden"))) int policy_act(const mjxPolicyDesc* desc, hipStream_t stream,
                                                     std::string* err);
}  // namespace mjx

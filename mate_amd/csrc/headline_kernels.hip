// headline_kernels.hip -- headline_rollout_kernel (headline_kernels.hpp), both store forms, as a translation unit of its own: its kernel-resource remarks
// are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_headline.json).
#include <hip/hip_runtime.h>
#include "headline_kernels.hpp"

namespace mate {

StepFn headline_rollout_function(int shifted) {
#if defined(MATE_PHASE_CLOCKS)
    (void)shifted;
    return nullptr;
#else
    return shifted ? (StepFn)headline_rollout_kernel<true> : (StepFn)headline_rollout_kernel<false>;
#endif
}

}  // namespace mate

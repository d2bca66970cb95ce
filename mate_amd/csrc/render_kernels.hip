// render_kernels.hip -- render_kernel's two instantiations and its launch function (render_rows.hpp describes them), as a translation unit of its own: its
// kernel-resource remarks are kept apart from every pinned record (mate_amd/build.py: lib/render_resources.json).
#include <hip/hip_runtime.h>
#include "render_rows.hpp"

namespace mate {

hipError_t launch_render(bool wide, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const RenderArgs &a) {
    if (wide) hipLaunchKernelGGL(render_kernel<true>, dim3(blocks), dim3(256), lds, stream, params, a);
    else hipLaunchKernelGGL(render_kernel<false>, dim3(blocks), dim3(256), lds, stream, params, a);
    return hipGetLastError();
}

}  // namespace mate

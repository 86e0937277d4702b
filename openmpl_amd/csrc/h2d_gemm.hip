// Direct-W form of the 16-row teams of the fp16x2 block stack (h2_stackd_kernel: form 2 of h2_stack_walk.inc), a translation unit of its own
// so that it compiles beside h2_gemm.hip / h2n_gemm.hip.
#include "h2_phase.hpp"

namespace mpl {

int launch_h2d_stack(const H2StackArgs& a, int grid, hipStream_t s) {
    if (int rc = kernel_lds_once<h2_stackd_kernel<2>>(H2_LDS_BYTES, 512)) return rc;
    if (a.rgs != 1) return MPL_E_INVALID;
    hipLaunchKernelGGL(h2_stackd_kernel<2>, dim3(grid), dim3(512), H2_LDS_BYTES, s, a);
    return MPL_OK;
}

}  // namespace mpl

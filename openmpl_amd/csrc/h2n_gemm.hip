// Row-narrow form of the fp16x2 block stack (h2_stackn_kernel: form 1 of h2_stack_walk.inc), a translation unit of its own so that it compiles
// beside h2_gemm.hip: the persistent stack kernel for launches that would leave most of the chip idle -- the reference's
// shipped call shape (configs/h36m/mpl_amass/h36m.yaml:37-39,107: TEST.BATCH_SIZE 256, two views; loop
// lib/core/function_mpl.py:334-351) is 512 token rows = 8 row tiles x 4 column groups = 32 of 256 compute units for
// h2_stack_kernel, which walks them in the 0.83 ms it needs for ANY number of tiles.  Here a 64-row tile is shared by 4 (2)
// teams of 16 (32) rows; same arithmetic per output element, bitwise the same poses (tests/test_h2_gpu.py).
#include "h2_phase.hpp"

namespace mpl {

int launch_h2n_stack(const H2StackArgs& a, int grid, hipStream_t s) {
    if (int rc = kernel_lds_once<h2_stackn_kernel<2>>(H2_LDS_BYTES, 512)) return rc;
    if (a.rgs != 1 && a.rgs != 2) return MPL_E_INVALID;
    hipLaunchKernelGGL(h2_stackn_kernel<2>, dim3(grid), dim3(512), H2_LDS_BYTES, s, a);
    return MPL_OK;
}

}  // namespace mpl

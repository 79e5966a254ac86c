// The path tracer's two ray kernels once more, compiled with -ffp-contract=fast (Makefile: variantC<ST>.o, -DFRAY_ARITH=1): multiply-add pairs of the
// FP64 geometry fuse into v_fma_f64.  The reference's build has no FMA (x86-64 baseline), so these kernels do NOT reproduce its bits; they are used,
// when a scene's option "fp_contract" is 1, only for what north_star bounds by colour (1e-4 RMS per channel): every bounce AFTER a camera sample's
// first closest hit, and every next-event visibility query.  Primary hit records (MODE_PRIMARY_ID) and a sample's first bounce never run here.
#ifndef FRAY_ARITH
#error "compile with -DFRAY_ARITH=1 -ffp-contract=fast"
#endif
#include "render_state.hpp"
#include "kernels.hpp"

#ifndef FRAY_ST
#error "compile with -DFRAY_ST=0..5, 8 or 9"
#endif

namespace frayhip_detail {
template <int ST> void launch_bounce_contracted(int grid, hipStream_t stream, const BounceArgs& A)
{
    hipLaunchKernelGGL((k_pt_bounce<ST, false, false, FRAY_ARITH>), dim3(grid), dim3(256), 0, stream, A);
}
template <int ST> void launch_shadow_contracted(int grid, hipStream_t stream, const ShadowArgs& A)
{
    hipLaunchKernelGGL((k_pt_shadow<ST, FRAY_ARITH>), dim3(grid), dim3(256), 0, stream, A);
}
template void launch_bounce_contracted<FRAY_ST>(int, hipStream_t, const BounceArgs&);
template void launch_shadow_contracted<FRAY_ST>(int, hipStream_t, const ShadowArgs&);
}

#if FRAY_ST == 0
// Test hook frayhip_debug_arith (include/frayhip.h): the relaxed primitives of this build -- the very inline functions the kernels above call, under the same
// -ffp-contract=fast -DFRAY_ARITH=1 -- on caller-supplied operands, so that a test can measure them against high-precision references.  Compiled once (flag word 0).
static __global__ __launch_bounds__(256) void k_debug_arith(int op, int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out)
{
#ifdef __HIP_DEVICE_COMPILE__          // (fray_rsqrt exists in the device pass only)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        switch (op) {
            case 0: out[i] = fray_rcp(a[i]); break;
            case 1: out[i] = fray_div(a[i], b[i]); break;
            case 2: out[i] = fray_rsqrt(a[i]); break;
            case 3: out[i] = fray_sqrt(a[i]); break;
            case 4: case 5: {
                V3 v = ld3(a + 3 * (size_t)i);
                if (op == 4) v = normalized(v);
                else { v = ld3(b + 3 * (size_t)i) - v; v = v * fray_rcp(length(v)); }          // visible(a, b): the segment's direction
                out[3 * (size_t)i] = v.x; out[3 * (size_t)i + 1] = v.y; out[3 * (size_t)i + 2] = v.z;
                break;
            }
            case 6: fray_sincos(a[i], &out[2 * (size_t)i], &out[2 * (size_t)i + 1]); break;
            case 7: fray_acos_sincos(a[i], &out[2 * (size_t)i], &out[2 * (size_t)i + 1]); break;
        }
    }
#endif
}

extern "C" int frayhip_debug_arith(int op, int n, const double* a, const double* b, double* out)
{
    using frayhip_detail::set_error;
    // doubles per item: operand a, operand b, result
    static const int kA[8] = {1, 1, 1, 1, 3, 3, 1, 1}, kB[8] = {0, 1, 0, 0, 0, 3, 0, 0}, kOut[8] = {1, 1, 1, 1, 3, 3, 2, 2};
    if (op < 0 || op > 7 || n <= 0 || n > (1 << 22) || !a || !out || (kB[op] && !b)) { set_error("frayhip_debug_arith: bad argument"); return FRAYHIP_E_ARG; }
    const size_t na = (size_t)n * kA[op], nb = (size_t)n * kB[op], no = (size_t)n * kOut[op];
    double* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, (na + nb + no) * 8));
    int rc = FRAYHIP_OK;
    if (hipMemcpy(d, a, na * 8, hipMemcpyHostToDevice) != hipSuccess || (nb && hipMemcpy(d + na, b, nb * 8, hipMemcpyHostToDevice) != hipSuccess)) rc = FRAYHIP_E_NODEVICE;
    if (rc == FRAYHIP_OK) {
        hipLaunchKernelGGL(k_debug_arith, dim3(frayhip_detail::grid_for(n)), dim3(256), 0, nullptr, op, n, d, nb ? d + na : nullptr, d + na + nb);
        if (hipDeviceSynchronize() != hipSuccess) rc = FRAYHIP_E_NODEVICE;
    }
    if (rc == FRAYHIP_OK && hipMemcpy(out, d + na + nb, no * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = FRAYHIP_E_NODEVICE;
    (void)hipFree(d);
    if (rc != FRAYHIP_OK) set_error("frayhip_debug_arith: device error");
    return rc;
}
#endif

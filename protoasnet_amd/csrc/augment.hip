// augment.hip -- the train-split augmentation of the reference's dataset (as_dataloader.py:127-133, 221-224) plus its normalisation,
// on the device, in one pass from the raw single-channel clip to the normalised one the training pass reads:
//   1. RandomResizedCropVideo (torchvision _transforms_video): crop clip[..., i:i+h, j:j+w], then
//      F.interpolate(size=(Ho, Wo), mode="bilinear", align_corners=False), no antialias:
//          source row  sy = max(0, (yo + 0.5) * (h / Ho) - 0.5),  y0 = (int)sy,  y1 = y0 + (y0 < h - 1),  ly = sy - y0  (columns alike)
//      (sy exact: integer part and remainder of ((2 yo + 1) h - Ho) / (2 Ho))
//   2. RandomRotateVideo (video_transforms.py:6-35): TF.rotate(angle, NEAREST, expand=False, fill=0) on the resized Ho x Wo grid.
//      rotate() passes -angle to _get_inverse_affine_matrix (the opposite sign of affine(), which warp.hip implements), so
//          centred output pixel (xc, yc) = (x - Wo/2 + 0.5, y - Ho/2 + 0.5)
//          source (xs, ys) = (cos t * xc - sin t * yc, sin t * xc + cos t * yc) + (Wo/2 - 0.5, Ho/2 - 0.5)
//      rounded half to even (grid_sample's nearbyint); a source outside the grid is the pixel value 0.
//   3. bin_to_norm (as_dataloader.py:173-182): (v * scale - mean) / std, scale 1/255 for uint8 clips.
// The parameters are per clip and the same for every frame: the coordinates and bilinear weights are computed once per (n, y, x) and the
// thread marches along T.  HBM-bound gather (the four taps of neighbouring outputs share cache lines).
#include "common.h"

namespace pasn {

struct AugParam {
    int i, j, h, w;
    float c, s;
};

__device__ __forceinline__ AugParam aug_param(const void* p, int n, int pcode) {
    if (pcode == PASN_F32) {
        const float* f = static_cast<const float*>(p) + (long)n * 6;
        return AugParam{(int)f[0], (int)f[1], (int)f[2], (int)f[3], f[4], f[5]};
    }
    const int* q = static_cast<const int*>(p) + (long)n * 6;
    return AugParam{q[0], q[1], q[2], q[3], __int_as_float(q[4]), __int_as_float(q[5])};
}

// one axis of the crop + bilinear resize: output index o of `out` samples -> the two source indices (absolute, clamped into [0, full))
// and the weight of the upper one.  The source coordinate (o + 0.5) * len / out - 0.5 = ((2o + 1) len - out) / (2 out) is split into
// its integer part and remainder in integer arithmetic, so the weight carries ONE rounding (an fp32 coordinate near 200 would carry
// 1e-5 of error into it; the reference interpolates its float64 clip)
__device__ __forceinline__ void aug_axis(int o, int off, int len, int out, int full, int& a, int& b, float& l1) {
    len = max(len, 1);
    const int num = max((2 * o + 1) * len - out, 0), den = 2 * out;  // clamped at source coordinate 0
    const int i0 = min(num / den, len - 1);
    const int i1 = i0 + (i0 < len - 1 ? 1 : 0);
    l1 = i0 == num / den ? __fdiv_rn((float)(num - i0 * den), (float)den) : 0.0f;
    a = min(max(off + i0, 0), full - 1);  // a table outside the clip reads its border instead of another clip's memory
    b = min(max(off + i1, 0), full - 1);
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void clip_augment_kernel(const TI* __restrict__ x, TO* __restrict__ y, const void* __restrict__ params,
                                                           int pcode, int N, int T, int H, int W, int Ho, int Wo, float scale, float mean,
                                                           float stdev) {
    const long total = (long)N * Ho * Wo;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int xo = (int)(idx % Wo), yo = (int)((idx / Wo) % Ho), n = (int)(idx / ((long)Ho * Wo));
        const AugParam p = aug_param(params, n, pcode);
        // 2. rotation: the nearest pixel of the resized grid this output takes
        const float xc = (float)xo - 0.5f * Wo + 0.5f, yc = (float)yo - 0.5f * Ho + 0.5f;
        const float xr = rintf(p.c * xc - p.s * yc + (0.5f * Wo - 0.5f));
        const float yr = rintf(p.s * xc + p.c * yc + (0.5f * Ho - 0.5f));
        const bool in = xr >= 0.0f && xr < (float)Wo && yr >= 0.0f && yr < (float)Ho;
        // 1. crop + bilinear resize at that pixel
        int r0, r1, c0, c1;
        float ly, lx;
        aug_axis(in ? (int)yr : 0, p.i, p.h, Ho, H, r0, r1, ly);
        aug_axis(in ? (int)xr : 0, p.j, p.w, Wo, W, c0, c1, lx);
        const float hy0 = 1.0f - ly, wx0 = 1.0f - lx;
        const long o00 = (long)r0 * W + c0, o01 = (long)r0 * W + c1, o10 = (long)r1 * W + c0, o11 = (long)r1 * W + c1;
        const TI* src = x + (long)n * T * H * W;
        TO* dst = y + (long)n * T * Ho * Wo + (long)yo * Wo + xo;
#pragma unroll 4  // four frames' gathers in flight per thread
        for (int t = 0; t < T; ++t) {
            float v = 0.0f;
            if (in) {
                const TI* f = src + (long)t * H * W;
                // taps to [0, 1] first (the reference resizes the [0, 1] clip); one rounding each, as torch's x * scale
                const float v00 = __fmul_rn((float)f[o00], scale), v01 = __fmul_rn((float)f[o01], scale);
                const float v10 = __fmul_rn((float)f[o10], scale), v11 = __fmul_rn((float)f[o11], scale);
                v = hy0 * (wx0 * v00 + lx * v01) + ly * (wx0 * v10 + lx * v11);  // upsample_bilinear2d's order
            }
            // 3. normalisation without contraction: identity parameters reproduce (x * scale - mean) / std bit for bit
            dst[(long)t * Ho * Wo] = (TO)__fdiv_rn(__fsub_rn(v, mean), stdev);
        }
    }
}

}  // namespace pasn

using namespace pasn;

extern "C" int pasn_clip_augment(const void* x, void* y, const void* params, int N, int T, int H, int W, int Ho, int Wo, float scale,
                                 float mean, float stdev, int in_dtype, int out_dtype, int param_dtype, void* stream) {
    PASN_REQUIRE(x && y && params && N > 0 && T > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "bad arguments");
    PASN_REQUIRE(stdev != 0.0f, "std must be non-zero");
    PASN_REQUIRE(in_dtype == PASN_F32 || in_dtype == PASN_BF16 || in_dtype == PASN_U8, "clip dtype is fp32, bf16 or uint8");
    PASN_REQUIRE(out_dtype == PASN_F32 || out_dtype == PASN_BF16, "output dtype is fp32 or bf16");
    PASN_REQUIRE(param_dtype == PASN_F32 || param_dtype == PASN_I32, "parameter table is fp32 or int32");
    const long total = (long)N * Ho * Wo;
    const int blocks = (int)std::min<long>((total + 255) / 256, 1 << 20);
    hipStream_t s = (hipStream_t)stream;
#define AUG(TI, TO)                                                                                                                     \
    hipLaunchKernelGGL((clip_augment_kernel<TI, TO>), dim3(blocks), dim3(256), 0, s, (const TI*)x, (TO*)y, params, param_dtype, N, T, H, \
                       W, Ho, Wo, scale, mean, stdev)
    if (in_dtype == PASN_U8) {
        if (out_dtype == PASN_BF16) AUG(uint8_t, __bf16);
        else AUG(uint8_t, float);
    } else if (in_dtype == PASN_BF16) {
        if (out_dtype == PASN_BF16) AUG(__bf16, __bf16);
        else AUG(__bf16, float);
    } else {
        if (out_dtype == PASN_BF16) AUG(float, __bf16);
        else AUG(float, float);
    }
#undef AUG
    return check_launch("clip_augment");
}

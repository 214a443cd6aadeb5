// One separable layer of MobileNet-v1 as ONE launch on gfx950 (WZ_OP_DWSEP):
//   depthwise 3x3 + BN + ReLU6 -> 1x1 pointwise + BN + ReLU6, fp16 NHWC in and out
//
// Unfused, the layer is wz_k_dw then wz_k_conv (k_conv.hip): two launches, and the depthwise output goes out to HBM and is read
// straight back.  Here it never leaves the CU:
//   * a workgroup (4 waves) owns 16 * MT consecutive output pixels of the batch and computes their depthwise outputs for ALL
//     cin channels once, into LDS as fp16 ([pixel][cin + 8]: 16-byte rows, no power-of-two pitch) -- exactly the B-operand
//     fragments of the pointwise GEMM (lane = pixel, 8 consecutive channels = one 16-byte LDS read);
//   * its waves then take column slices of the output: wave w of column group blockIdx.y owns the 16-column tiles
//     (blockIdx.y * 4 + w) * NTW .. + NTW - 1 for all MT pixel tiles.  K (= cin) is never split: no workspace, no reduce launch;
//   * epilogue: + bias, ReLU6, fp16 NHWC store.
// Up to 1024 output columns are 64 tiles: too many accumulators for one wave, hence the column groups over workgroups (each
// recomputes the depthwise part of its pixels: 9 FMAs per channel against 64 * NTW MACs on the matrix cores).
//
// Rounding and order are the unfused kernels': the depthwise sum starts from the bias and runs fmaf over ky, then kx, skipping
// taps outside the image (wz_k_dw), one fp16 rounding after ReLU6; the pointwise sum takes K chunks of 32 in order 0 .. kc - 1
// into one fp32 accumulator per fragment (v_mfma_f32_16x16x32_f16, weights as the A operand) and finishes with wz_epilogue4's
// arithmetic.  Both programs therefore produce bit-identical tensors when the unfused conv is not split along K
// (tests/test_gpu_mobilenet_v1.py, WZ_SPLITK=0).
#include "wz_common.h"

template <int MT, int NTW>
__global__ __launch_bounds__(256) void wz_k_dwsep(const WzDwsepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wz_dwsep_smem[];
    half_t* const X = reinterpret_cast<half_t*>(wz_dwsep_smem);   // [16 * MT][es]
    WZ_LANE_STAMP(a.dbg);
    const int es = a.cin + 8;
    const int m0 = blockIdx.x * 16 * MT;

    // ---- depthwise: item = (pixel, group of 8 channels), channel-fastest for coalesced loads
    {
        const int c8 = a.cin >> 3;
        const int hw = a.hout * a.wout;
        for (int i = threadIdx.x; i < 16 * MT * c8; i += 256) {
            const int px = i / c8, cg = i - px * c8;
            const int m = m0 + px;
            half8_t o = {0, 0, 0, 0, 0, 0, 0, 0};   // (pixels beyond the batch: computed on nothing, never stored)
            if (m < a.M) {
                const int b = m / hw, pix = m - b * hw;
                const int oy = pix / a.wout, ox = pix - oy * a.wout;
                float acc[8];
                const float4_t b0 = *reinterpret_cast<const float4_t*>(a.bd + cg * 8);
                const float4_t b1 = *reinterpret_cast<const float4_t*>(a.bd + cg * 8 + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc[j] = b0[j]; acc[4 + j] = b1[j]; }
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int iy = oy * a.stride - a.pad_t + ky;
                    if (iy < 0 || iy >= a.hin) continue;
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ix = ox * a.stride - a.pad_l + kx;
                        if (ix < 0 || ix >= a.win) continue;
                        const half8_t x = *reinterpret_cast<const half8_t*>(a.in + ((size_t)(b * a.hin + iy) * a.win + ix) * a.cin + cg * 8);
                        const half8_t k = *reinterpret_cast<const half8_t*>(a.wd + (size_t)(ky * 3 + kx) * a.cin + cg * 8);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] = fmaf((float)x[j], (float)k[j], acc[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = (half_t)fminf(fmaxf(acc[j], 0.0f), 6.0f);
            }
            *reinterpret_cast<half8_t*>(X + px * es + cg * 8) = o;
        }
    }
    __syncthreads();

    // ---- pointwise: this wave's NTW column tiles for the MT pixel tiles, K chunks in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int nt0 = (blockIdx.y * 4 + wave) * NTW;
    float4_t acc[MT][NTW];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = (float4_t){0.f, 0.f, 0.f, 0.f};
    const half_t* const wsrc = a.wp + ((size_t)nt0 * a.kc * 64 + lane) * 8;   // fragment (nt0 + nt, kk) at + (nt * kc + kk) * 512
    half8_t wa[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) wa[nt] = *reinterpret_cast<const half8_t*>(wsrc + (size_t)nt * a.kc * 512);
    for (int kk = 0; kk < a.kc; ++kk) {
        const int kn = min(kk + 1, a.kc - 1);   // next step's weights in flight during this step's MFMAs (the last one reloads itself)
        half8_t wn[NTW];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) wn[nt] = *reinterpret_cast<const half8_t*>(wsrc + ((size_t)nt * a.kc + kn) * 512);
        half8_t bf[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) bf[mt] = *reinterpret_cast<const half8_t*>(X + (mt * 16 + r16) * es + kk * 32 + g * 8);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[nt], bf[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) wa[nt] = wn[nt];
    }

    // ---- epilogue: lane holds output channels n4 .. n4 + 3 of pixel m (wz_epilogue4's arithmetic with ReLU6, whole tensor, no residual)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m0 + mt * 16 + r16;
        if (m >= a.M) continue;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const int n4 = (nt0 + nt) * 16 + g * 4;
            if (n4 >= a.cout) continue;
            const float4_t bv = *reinterpret_cast<const float4_t*>(a.bp + n4);
            float4_t v = acc[mt][nt];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = fminf(fmaxf(v[r] + bv[r], 0.0f), 6.0f);
            const half4_t h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            *reinterpret_cast<half4_t*>(a.out + (size_t)m * a.cout + n4) = h;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// Pixel tiles per workgroup MT: enough (pixel, 8-channel) depthwise items for the 256 threads; it depends on cin alone.  Column tiles
// per wave NTW: a power of two that divides the layer's 64-column groups, at most 8 accumulator fragments per wave (MT * NTW <= 8), as
// large as keeps >= one workgroup per CU (256) in flight, and at least 2 where the output has them -- every column group recomputes
// the depthwise part of its pixels.  Only NTW depends on the batch, and every value it can take for a shape is one of the powers of two
// below the shape's largest: each is instantiated (wz_launch_dwsep), so a shape covered at batch 1 is covered at every batch.
static void wz_dwsep_choose(const WzDwsepArgs& a, int* mt, int* ntw) {
    *mt = a.cin <= 32 ? 4 : a.cin <= 64 ? 2 : 1;
    const int n_tiles = a.n_pad / 16, groups64 = a.n_pad / 64;
    const long mgroups = ((long)a.M + 16 * *mt - 1) / (16 * *mt);
    int t = 1;
    while (2 * t * *mt <= 8 && groups64 % (2 * t) == 0) t *= 2;
    while (t > 2 && mgroups * (n_tiles / (4 * t)) < 256) t /= 2;
    *ntw = t;
}

// The shapes this kernel covers (the load-time check and the launch evaluate the same predicate): K in whole 32-channel chunks
// (32 .. 1024: the LDS tile holds 16 * MT pixels x cin channels), whole 64-column groups, 3x3 stride 1 / 2 with TF 'SAME' padding.
static bool wz_dwsep_covered(const WzDwsepArgs& a) {
    return a.cin >= 32 && a.cin <= 1024 && a.cin % 32 == 0 && a.kc == a.cin / 32 && a.n_pad % 64 == 0 && a.n_pad >= a.cout &&
           a.cout % 8 == 0 && a.cout > 0 && (a.stride == 1 || a.stride == 2) && a.hout == (a.hin + a.stride - 1) / a.stride &&
           a.wout == (a.win + a.stride - 1) / a.stride && a.pad_t >= 0 && a.pad_t <= 1 && a.pad_l >= 0 && a.pad_l <= 1 && a.M > 0;
}

template <int MT, int NTW>
static int wz_dwsep_launch(const WzDwsepArgs& a, hipStream_t s, bool prepare) {
    const size_t lds = (size_t)16 * MT * (a.cin + 8) * sizeof(half_t);
    if (lds > 64 * 1024) return -1;
    if (prepare) return 0;
    const int groups = a.n_pad / (64 * NTW);
    WZ_LAUNCH((wz_k_dwsep<MT, NTW>), dim3((a.M + 16 * MT - 1) / (16 * MT), groups), dim3(256), lds, s, a);
    return 0;
}

// prepare = true: evaluate the predicate and the configuration, launch nothing (engine creation; n = 1).  Returns -1 for a shape
// the predicate does not cover (the engine then refuses the file), else 0.  The instantiations are every (MT, NTW) wz_dwsep_choose can
// return: MT * NTW <= 8, NTW a power of two.
int wz_launch_dwsep(const WzDwsepArgs& a, hipStream_t s, bool prepare) {
    if (!wz_dwsep_covered(a)) return -1;
    int mt, ntw;
    wz_dwsep_choose(a, &mt, &ntw);
#define WZ_DWSEP_CASE(M_, N_) \
    if (mt == M_ && ntw == N_) return wz_dwsep_launch<M_, N_>(a, s, prepare)
    WZ_DWSEP_CASE(4, 1);
    WZ_DWSEP_CASE(4, 2);
    WZ_DWSEP_CASE(2, 1);
    WZ_DWSEP_CASE(2, 2);
    WZ_DWSEP_CASE(2, 4);
    WZ_DWSEP_CASE(1, 1);
    WZ_DWSEP_CASE(1, 2);
    WZ_DWSEP_CASE(1, 4);
    WZ_DWSEP_CASE(1, 8);
#undef WZ_DWSEP_CASE
    return -1;
}

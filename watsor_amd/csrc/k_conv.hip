// Convolution stack of SSD-MobileNet-v2 on gfx950: activations NHWC fp16 in HBM, fp32 accumulate.
//
// In the reference all of this is inside `sess.run` (`watsor/detection/tensorflow_cpu.py:114-115`)
// or inside the TensorRT engine (`tensorrt_gpu.py:150`); there is no reference kernel to mirror
// (SURVEY.md §2 "Native inventory").  Layer shapes: SURVEY.md Appendix A.
//
//  wz_k_stem   3x3 s2, 3(+1 pad)->32, BN folded, ReLU6            VALU, K = 27
//  wz_k_dw     depthwise 3x3 s1/s2, TF SAME, BN folded, ReLU6      VALU, HBM-bound (AI 1.8-4.5 flop/B)
//  wz_k_conv   1x1 and dense 3x3 as implicit GEMM on v_mfma_f32_16x16x32_f16:
//              D[n][m] = sum_k W[n][k] * X[m][k]; the weights are the MFMA "A" operand (pre-packed by
//              the engine builder in fragment order, one coalesced 1 KiB load per fragment) and the
//              activations the "B" operand (each lane gathers 8 consecutive channels = 16 B of one
//              input pixel), so a lane ends up with 4 consecutive output channels of one pixel and
//              stores them as one 8-byte word.  Epilogue fuses bias, ReLU6 and the residual add.
//  wz_k_splitk_reduce  deterministic (fixed order) reduction of split-K partials + the same epilogue.
#include "wz_common.h"

// --------------------------------------------------------------------------------------------
// stem: thread = (output pixel, group of 8 output channels)
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wz_k_stem(const half_t* __restrict__ in, const float* __restrict__ w,
                                                 const float* __restrict__ bias, half_t* __restrict__ out,
                                                 int total, int hin, int win, int hout, int wout, int pad_t,
                                                 int pad_l) {
    __shared__ float sw[27 * 32 + 32];
    for (int i = threadIdx.x; i < 27 * 32; i += 256) sw[i] = w[i];
    if (threadIdx.x < 32) sw[27 * 32 + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= total) return;
    const int cg = tid & 3, pix = tid >> 2;
    const int ox = pix % wout;
    const int t2 = pix / wout;
    const int oy = t2 % hout, b = t2 / hout;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = sw[27 * 32 + cg * 8 + j];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - pad_t + ky;
        if (iy < 0 || iy >= hin) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - pad_l + kx;
            if (ix < 0 || ix >= win) continue;
            const half4_t p = *reinterpret_cast<const half4_t*>(in + ((size_t)(b * hin + iy) * win + ix) * 4);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = (float)p[c];
                const float* wr = sw + ((ky * 3 + kx) * 3 + c) * 32 + cg * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(x, wr[j], acc[j]);
            }
        }
    }
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (half_t)fminf(fmaxf(acc[j], 0.0f), 6.0f);
    *reinterpret_cast<half8_t*>(out + (size_t)pix * 32 + cg * 8) = o;
}

void wz_launch_stem(const half_t* in, const float* w, const float* bias, half_t* out, int n, int hin, int win,
                    int hout, int wout, int pad_t, int pad_l, hipStream_t s) {
    const int total = n * hout * wout * 4;
    WZ_LAUNCH(wz_k_stem, dim3((total + 255) / 256), dim3(256), 0, s, in, w, bias, out, total, hin, win,
                       hout, wout, pad_t, pad_l);
}

// --------------------------------------------------------------------------------------------
// depthwise 3x3: thread = (output pixel, group of 8 channels); 16-byte loads/stores, channel-coalesced
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wz_k_dw(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                               const float* __restrict__ bias, half_t* __restrict__ out,
                                               int total, int hin, int win, int c, int hout, int wout, int stride,
                                               int pad_t, int pad_l, int act) {
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= total) return;
    const int c8 = c >> 3;
    const int cg = tid % c8, pix = tid / c8;
    const int ox = pix % wout;
    const int t2 = pix / wout;
    const int oy = t2 % hout, b = t2 / hout;
    float acc[8];
    {
        const float4_t b0 = *reinterpret_cast<const float4_t*>(bias + cg * 8);
        const float4_t b1 = *reinterpret_cast<const float4_t*>(bias + cg * 8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[j] = b0[j]; acc[4 + j] = b1[j]; }
    }
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - pad_t + ky;
        if (iy < 0 || iy >= hin) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - pad_l + kx;
            if (ix < 0 || ix >= win) continue;
            const half8_t x = *reinterpret_cast<const half8_t*>(in + ((size_t)(b * hin + iy) * win + ix) * c + cg * 8);
            const half8_t k = *reinterpret_cast<const half8_t*>(w + (size_t)(ky * 3 + kx) * c + cg * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = fmaf((float)x[j], (float)k[j], acc[j]);
        }
    }
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float v = acc[j];
        if (act == WZ_ACT_RELU6) v = fminf(fmaxf(v, 0.0f), 6.0f);
        o[j] = (half_t)v;
    }
    *reinterpret_cast<half8_t*>(out + (size_t)pix * c + cg * 8) = o;
}

void wz_launch_dw(const half_t* in, const half_t* w, const float* bias, half_t* out, int n, int hin, int win,
                  int c, int hout, int wout, int stride, int pad_t, int pad_l, int act, hipStream_t s) {
    const int total = n * hout * wout * (c >> 3);
    WZ_LAUNCH(wz_k_dw, dim3((total + 255) / 256), dim3(256), 0, s, in, w, bias, out, total, hin, win, c,
                       hout, wout, stride, pad_t, pad_l, act);
}

// --------------------------------------------------------------------------------------------
// implicit-GEMM convolution on MFMA.  Workgroup = 4 waves; wave = (MT*16 pixels) x (NT*16 channels).
// --------------------------------------------------------------------------------------------

// (wz_epilogue4 -- bias, ReLU6, residual, the one fp16 rounding, the head scatter -- lives in wz_common.h: k_gemm_1x1.hip ends in it as well)

// The reductions of several convolutions in one launch: a workgroup finds its entry from the prefix table, then does
// exactly what wz_k_splitk_reduce does (same order over the splits: bit-identical results).
// box decode + clip of one anchor from its finished encoding (ty, tx, th, tw): the arithmetic of wz_k_decode
// (k_post.hip, which is compiled without contraction -- hence the pragma), operation for operation
__device__ __forceinline__ void wz_decode_anchor(const float4_t e, const float4_t an, const WzPostConsts& k,
                                                 float* __restrict__ box_out, uint8_t* __restrict__ valid_out) {
#pragma clang fp contract(off)
    const float ty = e[0] / k.scale_y, tx = e[1] / k.scale_x, th = e[2] / k.scale_h, tw = e[3] / k.scale_w;
    const float w = expf(tw) * an[3];
    const float h = expf(th) * an[2];
    const float yc = ty * an[2] + an[0];
    const float xc = tx * an[3] + an[1];
    const float hh = h / 2.0f, hw = w / 2.0f;
    float ymin = yc - hh, xmin = xc - hw, ymax = yc + hh, xmax = xc + hw;
    if (k.clip_after) {   // the NMS takes the boxes as decoded; every anchor is a candidate (wz_k_nms clips what it keeps)
        *reinterpret_cast<float4_t*>(box_out) = (float4_t){ymin, xmin, ymax, xmax};
        *valid_out = 1;
        return;
    }
    ymin = fminf(fmaxf(ymin, 0.0f), 1.0f);
    xmin = fminf(fmaxf(xmin, 0.0f), 1.0f);
    ymax = fminf(fmaxf(ymax, 0.0f), 1.0f);
    xmax = fminf(fmaxf(xmax, 0.0f), 1.0f);
    const float area = (ymax - ymin) * (xmax - xmin);
    *reinterpret_cast<float4_t*>(box_out) = (float4_t){ymin, xmin, ymax, xmax};
    *valid_out = area > 0.0f ? 1 : 0;
}

// Everything that happens to four finished output columns n4 .. n4+3 of pixel m of an SSD head (v = the K sum, bias not yet
// added): the epilogue proper (bias, store into the box-encoding / class-logit buffers), and optionally the candidate
// marking for wz_k_nms and the box decode.
__device__ __forceinline__ void wz_head_finish(const WzConvArgs& a, int m, int n4, float4_t v, bool list, bool decode,
                                               const float* __restrict__ hint_logit, uint32_t* __restrict__ cbits,
                                               int cbits_words, const WzPostConsts& pc, const float* __restrict__ anchors,
                                               float* __restrict__ boxes, uint8_t* __restrict__ valid) {
    wz_epilogue4(a, m, n4, v);
    if (m >= a.M) return;
    const int n_box = a.out_mode == WZ_OUT_HEAD ? a.n_box : (a.out_mode == WZ_OUT_BOX ? a.cout : 0);
    if (list && n4 >= n_box && n4 < a.cout && a.out_mode != WZ_OUT_BOX && a.out_mode != WZ_OUT_ACT) {
        // class logits of one anchor location, four at a time: the ones that can reach the frame's first score band
        // are listed for wz_k_nms (which re-derives score, validity and bin exactly as its own scan would)
        const int hw = a.hout * a.wout;
        const int b = m / hw, pix = m - b * hw;
        const int cols = a.cout - n_box, n0 = n4 - n_box;
        const long long off = a.out_mode == WZ_OUT_HEAD ? a.out2_off : a.out_off;
        const float lf = hint_logit[b];
        const float4_t bv = *reinterpret_cast<const float4_t*>(a.bias + n4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float x = v[r] + bv[r];   // what the epilogue stored
            if (n0 + r < cols && x >= lf) {
                const long long j = off + (long long)pix * cols + n0 + r;   // entry index within the frame's logits
                atomicOr(&cbits[(size_t)b * cbits_words + (size_t)(j >> 5)], 1u << (j & 31));   // result unused
            }
        }
    }
    if (decode && n4 < n_box) {   // columns n4 .. n4+3 = the encoding of anchor (pixel, n4 / 4)
        const float4_t bv = *reinterpret_cast<const float4_t*>(a.bias + n4);
        float4_t enc;
#pragma unroll
        for (int r = 0; r < 4; ++r) enc[r] = v[r] + bv[r];   // what the epilogue stored
        const int hw = a.hout * a.wout;
        const int b = m / hw, pix = m - b * hw;
        const int anchor = (int)(a.out_off >> 2) + pix * (n_box >> 2) + (n4 >> 2);
        const size_t i = (size_t)b * pc.num_anchors + anchor;
        wz_decode_anchor(enc, *reinterpret_cast<const float4_t*>(anchors + (size_t)anchor * 4), pc, boxes + i * 4, valid + i);
    }
}


// Tile configuration: a wave computes (MT*16 pixels) x (NT*16 channels); U K-chunks (32 channels each)
// per register buffer, two buffers in flight.
//   <2,2,4>  small layers / small N: many waves, 1 KiB of loads per MFMA
//   <4,4,2>  the 3x3 SSD heads (M >= 128, N >= 256, K in the thousands): 4x the L2->register reuse
template <int MT, int NT, int U>
struct ConvFrags {
    half8_t xa[U][MT];
    half8_t wf[U][NT];
};

// Issue the loads of the next U K-chunks (flattened index ql = tap * kc + c) into `f`.
// (t, c) walk the chunk order; chunks at or beyond q1 load nothing and contribute zeros.
template <int KS, int MT, int NT, int U>
__device__ __forceinline__ void wz_conv_load(const WzConvArgs& a, ConvFrags<MT, NT, U>& f, int& ql, const int q1, int& t,
                                             int& c, const int (&iy0)[MT], const int (&ix0)[MT],
                                             const int (&boff)[MT], const bool (&mv)[MT],
                                             const half_t* wlane, const int nt0, const int cg8) {
    constexpr int taps = KS * KS;
    const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool live = ql < q1;   // wave-uniform
        const int ky = (KS == 1) ? 0 : t / KS, kx = (KS == 1) ? 0 : t - ky * KS;
        const bool cin_ok = (c * 32 + cg8) < a.cin;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int iy = iy0[mt] + ky, ix = ix0[mt] + kx;
            const bool ok = live && cin_ok && mv[mt] && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win;
            f.xa[u][mt] = ok ? *reinterpret_cast<const half8_t*>(
                                   a.in + ((size_t)(boff[mt] + iy) * a.win + ix) * a.cin + c * 32 + cg8)
                             : zero;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            f.wf[u][nt] = live ? *reinterpret_cast<const half8_t*>(
                                     wlane + ((size_t)((nt0 + nt) * taps + t) * a.kc + c) * 512)
                               : zero;
        ++ql;
        if (++c == a.kc) {
            c = 0;
            ++t;
        }
    }
}

template <int MT, int NT, int U>
__device__ __forceinline__ void wz_conv_mfma(const ConvFrags<MT, NT, U>& f, float4_t (&acc)[MT][NT]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(f.wf[u][nt], f.xa[u][mt], acc[mt][nt], 0, 0, 0);
}

template <int KS, int MT, int NT, int U>
__device__ __forceinline__ void wz_conv_body(const WzConvArgs& a, int bx, int by, int bz) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int m_base = (bx * 4 + wave) * (MT * 16);
    const int nt0 = by * NT;
    if (m_base >= a.M) return;   // whole wave out of range (no barriers in this kernel)

    const int hw = a.hout * a.wout;
    int iy0[MT], ix0[MT], boff[MT];
    bool mv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m_base + mt * 16 + r16;
        mv[mt] = m < a.M;
        const int mm = mv[mt] ? m : 0;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / a.wout, ox = rem - oy * a.wout;
        iy0[mt] = oy * a.stride - a.pad_t;
        ix0[mt] = ox * a.stride - a.pad_l;
        boff[mt] = b * a.hin;
    }

    float4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (float4_t){0.f, 0.f, 0.f, 0.f};

    // K range of this split (flattened chunk index q = tap * kc + c)
    const int per = (a.kchunks + a.splitk - 1) / a.splitk;
    const int q0 = bz * per;
    const int q1 = min(q0 + per, a.kchunks);
    const half_t* wlane = a.w + (size_t)lane * 8;
    const int cg8 = g * 8;

    // software pipeline: while the MFMAs of one register buffer run, the loads of the other are in flight
    int ql = q0, t = (KS == 1) ? 0 : q0 / a.kc, c = (KS == 1) ? q0 : q0 - t * a.kc;
    ConvFrags<MT, NT, U> fa, fb;
    wz_conv_load<KS, MT, NT, U>(a, fa, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
    for (int q = q0; q < q1;) {
        wz_conv_load<KS, MT, NT, U>(a, fb, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
        wz_conv_mfma(fa, acc);
        q += U;
        if (q >= q1) break;
        wz_conv_load<KS, MT, NT, U>(a, fa, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
        wz_conv_mfma(fb, acc);
        q += U;
    }

    // D layout: lane holds rows (n) g*4..g*4+3 of column (m) r16
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m_base + mt * 16 + r16;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int n4 = (nt0 + nt) * 16 + g * 4;
            if (a.splitk > 1) {
                if (m < a.M)
                    *reinterpret_cast<float4_t*>(reinterpret_cast<float*>(a.out) +
                                                 ((size_t)bz * a.M + m) * a.n_pad + n4) = acc[mt][nt];
            } else {
                wz_epilogue4(a, m, n4, acc[mt][nt]);
            }
        }
    }
}

template <int KS, int MT, int NT, int U>
__global__ __launch_bounds__(256) void wz_k_conv(const WzConvArgs a) {
    WZ_LANE_STAMP(a.dbg);
    wz_conv_body<KS, MT, NT, U>(a, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Split-K inside the workgroup, for the convolutions of the SSD extras chain (10x10 ... 1x1 maps, K up to 2 304, each
// feeding the next one): the 8 waves of a workgroup share ONE 32-pixel x 32-channel tile and each walks an eighth of
// the K chunks; the eight accumulator sets meet in LDS and are summed in wave order (deterministic).  No partial sums
// in HBM and no reduce launch behind the convolution -- on this chain a kernel boundary costs as much as the kernel.
// WM x WN: the workgroup's tile is WM x WN such 32 x 32 tiles and K is cut 8 / (WM WN) ways; U: K chunks per load group (two groups in flight);
// WGS_PER_CU = 2 holds the kernel to 128 registers (U = 2: 109) so that two workgroups share a CU (U = 4: 173 registers, a CU per workgroup).
template <int KS, int WM = 1, int WN = 1, int U = 2, int WGS_PER_CU = 2>
__global__ __launch_bounds__(512, WGS_PER_CU) void wz_k_conv_ws(const WzConvArgs a) {
    WZ_LANE_STAMP(a.dbg);
    constexpr int MT = 2, NT = 2, WAVES = 8, KSPL = WAVES / (WM * WN);
    static_assert(KSPL * WM * WN == WAVES, "eight waves: sub-tiles x K slices");
    __shared__ float4_t red[WAVES][MT * NT][64];   // 32 KiB
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int sub = wave / KSPL, ks = wave - sub * KSPL;   // which 32 x 32 tile of the workgroup's, which K slice of it
    const int m_base = ((int)blockIdx.x * WM + sub / WN) * (MT * 16);
    const int nt0 = ((int)blockIdx.y * WN + sub % WN) * NT;
    const bool tile_live = m_base < a.M && nt0 * 16 < a.n_pad;   // (wave-uniform; a dead tile still takes the barrier)

    const int hw = a.hout * a.wout;
    int iy0[MT], ix0[MT], boff[MT];
    bool mv[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = m_base + mt * 16 + r16;
        mv[mt] = m < a.M;
        const int mm = mv[mt] ? m : 0;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / a.wout, ox = rem - oy * a.wout;
        iy0[mt] = oy * a.stride - a.pad_t;
        ix0[mt] = ox * a.stride - a.pad_l;
        boff[mt] = b * a.hin;
    }
    float4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (float4_t){0.f, 0.f, 0.f, 0.f};

    const int per = (a.kchunks + KSPL - 1) / KSPL;
    const int q0 = ks * per, q1 = min(q0 + per, a.kchunks);
    if (tile_live && q0 < q1) {
        const half_t* wlane = a.w + (size_t)lane * 8;
        const int cg8 = g * 8;
        int ql = q0, t = (KS == 1) ? 0 : q0 / a.kc, c = (KS == 1) ? q0 : q0 - t * a.kc;
        ConvFrags<MT, NT, U> fa, fb;
        wz_conv_load<KS, MT, NT, U>(a, fa, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
        for (int q = q0; q < q1;) {
            wz_conv_load<KS, MT, NT, U>(a, fb, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
            wz_conv_mfma(fa, acc);
            q += U;
            if (q >= q1) break;
            wz_conv_load<KS, MT, NT, U>(a, fa, ql, q1, t, c, iy0, ix0, boff, mv, wlane, nt0, cg8);
            wz_conv_mfma(fb, acc);
            q += U;
        }
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) red[wave][mt * NT + nt][lane] = acc[mt][nt];
    __syncthreads();
    // K slice ks of a tile finishes its 16 x 16 sub-tiles ks, ks + KSPL, ...: the sum over the slices in slice order, then the epilogue
    // (eight slices: waves 0 .. 3 one sub-tile each, as before; two slices: two each)
    if (tile_live) {
        for (int tl = ks; tl < MT * NT; tl += KSPL) {
            float4_t v = red[sub * KSPL][tl][lane];
#pragma unroll
            for (int z = 1; z < KSPL; ++z) {
                const float4_t p = red[sub * KSPL + z][tl][lane];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += p[r];
            }
            wz_epilogue4(a, m_base + (tl / NT) * 16 + r16, (nt0 + tl % NT) * 16 + g * 4, v);
        }
    }
}

// Several small 3x3 convolutions that do not depend on each other (the SSD heads on the 3x3 ... 1x1 maps) in one launch:
// a workgroup finds its entry from the prefix table and runs wz_k_conv's body on it.
__global__ __launch_bounds__(256) void wz_k_conv_group(const WzConvGroup g) {
    WZ_LANE_STAMP(g.stamp);
    int e = 0;
    while (e + 1 < g.n && (int)blockIdx.x >= g.first[e + 1]) ++e;   // wave-uniform
    const int L = (int)blockIdx.x - g.first[e];
    const int gx = g.gx[e], gy = g.gy[e];
    wz_conv_body<3, 2, 2, 4>(g.a[e], L % gx, (L / gx) % gy, L / (gx * gy));
}

__global__ __launch_bounds__(256) void wz_k_splitk_reduce(const WzConvArgs a, const float* __restrict__ ws) {
    WZ_LANE_STAMP(a.dbg);
    const int tid = blockIdx.x * 256 + threadIdx.x;
    const int n4s = a.n_pad >> 2;
    if (tid >= a.M * n4s) return;
    const int m = tid / n4s, n4 = (tid - m * n4s) * 4;
    float4_t v = {0.f, 0.f, 0.f, 0.f};
    for (int z = 0; z < a.splitk; ++z) {
        const float4_t p = *reinterpret_cast<const float4_t*>(ws + ((size_t)z * a.M + m) * a.n_pad + n4);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += p[r];
    }
    wz_epilogue4(a, m, n4, v);
}

// The reductions of several convolutions in one launch: a workgroup finds its entry from the prefix table, then does
// exactly what wz_k_splitk_reduce does (same order over the splits: bit-identical results).
__global__ __launch_bounds__(256) void wz_k_splitk_reduce_group(const WzReduceGroup g) {
    WZ_LANE_STAMP(g.stamp);
    int e = 0;
    while (e + 1 < g.n && (int)blockIdx.x >= g.first[e + 1]) ++e;   // wave-uniform
    const WzConvArgs& a = g.a[e];
    const float* __restrict__ ws = g.ws[e];
    const int tid = ((int)blockIdx.x - g.first[e]) * 256 + threadIdx.x;
    int m, n4;
    size_t off, zstride;
    if (a.frag_ws) {   // partials in fragment order (WzConvArgs::frag_ws): a wavefront reads one 1 KiB fragment per slice
        const int mtt = (a.M + 15) >> 4, ntt = a.n_pad >> 4;
        const int frag = tid >> 6, lane = tid & 63;
        if (frag >= mtt * ntt) return;
        const int fm = frag / ntt;
        m = fm * 16 + (lane & 15);
        n4 = (frag - fm * ntt) * 16 + (lane >> 4) * 4;
        if (m >= a.M) return;
        off = (size_t)frag * 256 + lane * 4;
        zstride = (size_t)mtt * ntt * 256;
    } else {
        const int n4s = a.n_pad >> 2;
        if (tid >= a.M * n4s) return;
        m = tid / n4s;
        n4 = (tid - m * n4s) * 4;
        off = (size_t)m * a.n_pad + n4;
        zstride = (size_t)a.M * a.n_pad;
    }
    if (n4 >= a.cout) return;   // padding columns: nothing is stored for them (and the wide tile kernel does not write their partials)
    // the slices in groups of four: a group's loads are all requested before the first add (one memory latency per four slices instead of one
    // per slice -- the launch is bound by exactly that chain); the adds stay in slice order 0, 1, 2 ...: bit-identical sums
    float4_t v = {0.f, 0.f, 0.f, 0.f};
    for (int z0 = 0; z0 < a.splitk; z0 += 4) {
        float4_t p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            p[k] = z0 + k < a.splitk ? *reinterpret_cast<const float4_t*>(ws + (size_t)(z0 + k) * zstride + off) : (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (z0 + k < a.splitk) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += p[k][r];
            }
    }
    wz_head_finish(a, m, n4, v, g.list != 0, g.decode != 0, g.hint_logit, g.cbits, g.cbits_words, g.pc, g.anchors, g.boxes, g.valid);
}

// --------------------------------------------------------------------------------------------
// Tiled implicit GEMM for the layers with a long K loop (the 3x3 SSD heads, the 3x3 extras, Conv_1): workgroup = 128
// pixels x 64 or 128 channels, K step = 64 (two MFMA K chunks); the kernel is wz_k_conv_rs (k_conv_rs.h).
// --------------------------------------------------------------------------------------------
#define WZ_LDS_TM 128
// NW = 16-channel tiles per wave pair: 2 -> workgroup tile 128 x 64, 4 -> 128 x 128 (twice the MFMAs per byte staged)
#define WZ_LDS_TN(NW) (2 * (NW) * 16)

#include "k_conv_rs.h"

struct WzEpiF16 {
    static __device__ __forceinline__ void apply(const WzConvArgs& a, int m, int n4, float4_t v) { wz_epilogue4(a, m, n4, v); }
    static __device__ __forceinline__ float* partials(const WzConvArgs& a) { return reinterpret_cast<float*>(a.out); }
};

template <int KS, int NW>
__global__ __launch_bounds__(256, 2) void wz_k_conv_rs(const WzConvArgs a) {   // <= 256 registers: two waves per SIMD
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 16384];
    WZ_LANE_STAMP(a.dbg);
    wz_conv_rs_body<KS, NW, false, WzEpiF16>(a, smem, blockIdx.x);
}

// The SSD heads served by the register-staged tile kernel (the two big ones with 128 x 128 tiles, the 5x5 one with
// 128 x 64) in one launch: the workgroups of the later entries fill the CUs the first one's last round leaves idle, two
// workgroups share a CU and cover each other's stalls, and the kernel boundaries between them go away
// (measured for the two big heads: 32 us together against 23 + 26 us apart).
__global__ __launch_bounds__(256, 2) void wz_k_conv_rs_group(const WzConvGroup g) {
    WZ_LANE_STAMP(g.stamp);
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 16384];
    int e = 0;
    while (e + 1 < g.n && (int)blockIdx.x >= g.first[e + 1]) ++e;   // wave-uniform
    const int L = (int)blockIdx.x - g.first[e];
    if (g.gx[e] == 4)   // channel tiles per wave pair of this entry (wave-uniform)
        wz_conv_rs_body<3, 4, false, WzEpiF16>(g.a[e], smem, L);
    else
        wz_conv_rs_body<3, 2, false, WzEpiF16>(g.a[e], smem, L);
}

// the LDS-tiled kernel needs whole 64-column tiles, whole 2-chunk K steps and enough pixels to fill a tile
bool wz_conv_use_lds(const WzConvArgs& a) {
    static const int min_m = wz_dev_env_int("WZ_LDS_MIN_M", 128);
    static const int min_k = wz_dev_env_int("WZ_LDS_MIN_KCHUNKS", 8);
    return a.zeros && a.n_pad % 64 == 0 && a.kc % 2 == 0 && a.M >= min_m && a.kchunks >= min_k && a.cin % 32 == 0;
}

// 128 x 128 workgroup tiles where there are enough channels and pixels for them to pay
int wz_lds_nw(int M, int n_pad, int kchunks) {
    static const int force = wz_dev_env_int("WZ_LDS_NW", 0);
    if (force == 2 || force == 4) return force;
    return (n_pad >= 256 && M >= 512 && kchunks >= 64) ? 4 : 2;   // measured: the two big heads gain, Conv_1 (K = 320) loses
}

int wz_choose_splitk_lds(int M, int n_pad, int kchunks) {
    static const int target = wz_dev_env_int("WZ_LDS_WGS", 192);   // measured 64 .. 512: fewer, longer K slices win (less partial-sum traffic); 192 best
    const int tn = WZ_LDS_TN(wz_lds_nw(M, n_pad, kchunks));
    const int wgs = ((M + WZ_LDS_TM - 1) / WZ_LDS_TM) * ((n_pad + tn - 1) / tn);
    const int nsteps = kchunks / 2;
    int s = (target + wgs - 1) / wgs;
    if (s > nsteps / 4) s = nsteps / 4;   // >= 4 steps per split
    if (s > 32) s = 32;
    return s < 1 ? 1 : s;
}

// measured (profiles/): the 64x64 tile wins only where M is large enough to keep >= 1 wave per SIMD
// busy through a long K loop (BoxPredictor_0: M = n*361); at M = n*100 it is latency-bound and loses.
static inline bool wz_conv_big(int M, int n_pad, int kchunks) { return n_pad % 64 == 0 && n_pad >= 256 && M >= 2048 && kchunks >= 64; }

int wz_choose_splitk(int M, int n_pad, int kchunks) {
    // Long K loops on few waves are latency-bound: split K until there is about one wave per SIMD
    // (1024), keeping >= 8 chunks per split so the extra reduce launch stays amortised.
    const bool big = wz_conv_big(M, n_pad, kchunks);
    const int tm = big ? 64 : 32, tn = big ? 64 : 32;
    const long waves = (long)((M + tm - 1) / tm) * (n_pad / tn);
    static const int target = [] { const char* e = wz_dev_getenv("WZ_SPLITK_WAVES"); return (e && atoi(e) > 0) ? atoi(e) : 1024; }();
    static const int max_split = [] { const char* e = wz_dev_getenv("WZ_SPLITK_MAX"); return (e && atoi(e) > 0) ? atoi(e) : 16; }();
    if (kchunks < 32 || waves >= target) return 1;
    int s = (int)(target / (waves > 0 ? waves : 1));
    const int max_by_k = kchunks / 8;
    if (s > max_by_k) s = max_by_k;
    if (s > max_split) s = max_split;
    return s < 1 ? 1 : s;
}

template <int MT, int NT, int U>
static void wz_launch_conv_cfg(const WzConvArgs& a, hipStream_t s) {
    const int mtiles = (a.M + MT * 16 - 1) / (MT * 16);
    dim3 grid((mtiles + 3) / 4, a.n_pad / (NT * 16), a.splitk);
    if (a.ksize == 1)
        WZ_LAUNCH((wz_k_conv<1, MT, NT, U>), grid, dim3(256), 0, s, a);
    else
        WZ_LAUNCH((wz_k_conv<3, MT, NT, U>), grid, dim3(256), 0, s, a);
}

// the register-staged tile kernel (k_conv_rs.h); the LDS-DMA form of the same tile it replaced is described in DESIGN.md section 5
template <int KS, int NW>
static void wz_launch_conv_lds(const WzConvArgs& a, dim3 grid, hipStream_t s) {
    WZ_LAUNCH((wz_k_conv_rs<KS, NW>), grid, dim3(256), 0, s, a);
}

void wz_launch_conv(const WzConvArgs& a0, hipStream_t s) {
    if (wz_conv_use_lds(a0)) {
        WzConvArgs a = a0;
        a.grid_m = (a.M + WZ_LDS_TM - 1) / WZ_LDS_TM;
        const int nw = wz_lds_nw(a.M, a.n_pad, a.kchunks);
        a.grid_n = (a.n_pad + WZ_LDS_TN(nw) - 1) / WZ_LDS_TN(nw);
        dim3 grid(a.grid_m * a.grid_n * a.splitk);
        if (nw == 4) {
            if (a.ksize == 1)
                wz_launch_conv_lds<1, 4>(a, grid, s);
            else
                wz_launch_conv_lds<3, 4>(a, grid, s);
        } else {
            if (a.ksize == 1)
                wz_launch_conv_lds<1, 2>(a, grid, s);
            else
                wz_launch_conv_lds<3, 2>(a, grid, s);
        }
        return;
    }
    const WzConvArgs& a = a0;
    if (wz_conv_big(a.M, a.n_pad, a.kchunks))
        wz_launch_conv_cfg<4, 4, 2>(a, s);
    else
        wz_launch_conv_cfg<2, 2, 4>(a, s);
}

// small maps, a K loop long enough for eight slices, whole 32-channel tiles
bool wz_conv_ws_applies(const WzConvArgs& a) {
    static const int on = wz_dev_env_int("WZ_CONV_WS", 1);
    return on && a.out_mode == WZ_OUT_ACT && a.M <= 1024 && a.kchunks >= 8 && a.n_pad % 32 == 0;
}
void wz_launch_conv_ws(const WzConvArgs& a, hipStream_t s) {
    // Conv_1 of the MobileNet-v2 programs (320 -> 1 280) no longer arrives here from two frames on: the engine hands every convolution that
    // wz_gemm_1x1_applies() accepts (1x1, K staged = 320, N >= 1 024, M >= 200) to k_gemm_1x1.hip before it asks for K slices, at every larger M as
    // well (batches 11 .. 32 used to leave for the LDS tile kernel, 11 with a reduce launch behind it).  Conv_1 at ONE frame (M = 100) still takes the
    // 32 x 32 tiles below, and any other 1x1 with many pixels x many channels the 32 x 64 ones, which were chosen on Conv_1:
    // many pixels x many channels (800 x 1 280): 1 000 tiles of 32 x 32 at 173 registers are one workgroup per CU and FOUR
    // rounds of workgroups that each wait out their operands' latency (13.3 us with split weights, K = 640).  32 x 64 tiles, K in four slices,
    // two chunks per load group (109 registers: two workgroups per CU) are 500 workgroups in ONE round: 6.9 us then, 8.6 us when the GEMM kernel was
    // measured against it (profiles/gemm_1x1_kernel_stats_lanes1.txt).  Measured beside it
    // (profiles/r04_conv1_tiles.txt): 32 x 32 at 109 registers 8.1 us, 64 x 64 (K in halves) 11.9 us, 64 x 64 at 173 registers 12.8 us (260
    // workgroups on 256 CUs: a second round for four of them).  WZ_CONV_WS64=0: the 32 x 32 tiles everywhere.
    static const int wide_tiles = wz_dev_env_int("WZ_CONV_WS64", 1);
    if (wide_tiles && a.ksize == 1 && a.M >= 512 && a.n_pad >= 512 && a.n_pad % 64 == 0 && a.kchunks >= 8) {
        WZ_LAUNCH((wz_k_conv_ws<1, 1, 2>), dim3((a.M + 31) / 32, a.n_pad / 64), dim3(512), 0, s, a);
        return;
    }
    const dim3 grid((a.M + 31) / 32, a.n_pad / 32);
    // (two K chunks per load group, 109 registers, two workgroups per CU for every launch of this kernel since late round 4: with U = 4 and 173
    //  registers a workgroup owned its CU -- the extras chain's launches 4.5 / 6.0 -> 4.0 / 5.1 us and, with four lanes in flight, 46.9 -> 47.4 k
    //  frames/s: what a launch keeps other lanes' workgroups from using counts, profiles/r04_conv1_tiles.txt)
    if (a.ksize == 1)
        WZ_LAUNCH(wz_k_conv_ws<1>, grid, dim3(512), 0, s, a);
    else
        WZ_LAUNCH(wz_k_conv_ws<3>, grid, dim3(512), 0, s, a);
}

// the 3x3 convolutions wz_launch_conv would give to wz_k_conv<3, 2, 2, 4>
bool wz_conv_groupable(const WzConvArgs& a) {
    return a.ksize == 3 && !wz_conv_use_lds(a) && !wz_conv_big(a.M, a.n_pad, a.kchunks);
}
void wz_conv_group_add(WzConvGroup& g, const WzConvArgs& a) {
    const int i = g.n++;
    const int mtiles = (a.M + 31) / 32;
    g.a[i] = a;
    g.gx[i] = (mtiles + 3) / 4;
    g.gy[i] = a.n_pad / 32;
    g.first[i + 1] = g.first[i] + g.gx[i] * g.gy[i] * a.splitk;
    g.a[i].grid_m = g.gx[i];
    g.a[i].grid_n = g.gy[i];
}
void wz_launch_conv_group(const WzConvGroup& g, hipStream_t s) {
    WZ_LAUNCH(wz_k_conv_group, dim3(g.first[g.n]), dim3(256), 0, s, g);
}

// the convolutions wz_launch_conv would give to wz_k_conv_rs<3, 4>
bool wz_conv_rs_groupable(const WzConvArgs& a) {
    return a.ksize == 3 && wz_conv_use_lds(a);
}
// Returns the number of entries added (0: the group is full).  A head whose packed columns are an odd number of 64-column
// tiles (BoxPredictor_0: 320 = 2 x 128 + 64, BoxPredictor_1: 576 = 4 x 128 + 64) goes in as TWO entries -- the 128-column
// tiles and one 64-column tile behind them -- instead of rounding up to 128-column tiles (384 / 640 columns of MFMA work: 20 % /
// 11 % of it on padding).  Both write the same partial-sum slab ([z][M][n_pad], absolute columns) with the same split count.
int wz_conv_rs_group_add(WzConvGroup& g, const WzConvArgs& a0) {
    static const int split_n = wz_dev_env_int("WZ_HEAD_SPLIT_N", 1);
    const int nw = wz_lds_nw(a0.M, a0.n_pad, a0.kchunks);
    const bool two = split_n && nw == 4 && (a0.n_pad % 128) == 64 && a0.n_pad > 128;
    if (g.n + (two ? 2 : 1) > WZ_CONV_GROUP_MAX) return 0;
    for (int part = 0; part < (two ? 2 : 1); ++part) {
        const int i = g.n++;
        WzConvArgs& a = g.a[i];
        a = a0;
        const int pnw = (two && part == 1) ? 2 : nw;
        a.grid_m = (a.M + WZ_LDS_TM - 1) / WZ_LDS_TM;
        a.nt_base = (two && part == 1) ? (a.n_pad / 128) * 8 : 0;
        a.grid_n = two ? (part == 0 ? a.n_pad / 128 : 1) : (a.n_pad + WZ_LDS_TN(nw) - 1) / WZ_LDS_TN(nw);
        g.gx[i] = pnw;
        g.gy[i] = 0;
        g.first[i + 1] = g.first[i] + ((a.grid_m * a.grid_n * a.splitk + 7) & ~7);   // entries start on an XCD boundary
    }
    return two ? 2 : 1;
}
void wz_launch_conv_rs_group(const WzConvGroup& g, hipStream_t s) {
    WZ_LAUNCH(wz_k_conv_rs_group, dim3(g.first[g.n]), dim3(256), 0, s, g);
}

void wz_reduce_group_add(WzReduceGroup& g, const WzConvArgs& a, const float* ws) {
    const int i = g.n++;
    g.a[i] = a;
    g.ws[i] = ws;
    const int threads = a.frag_ws ? ((a.M + 15) >> 4) * (a.n_pad >> 4) * 64 : a.M * (a.n_pad >> 2);
    g.first[i + 1] = g.first[i] + (threads + 255) / 256;
}
void wz_launch_splitk_reduce_group(const WzReduceGroup& g, hipStream_t s) {
    WZ_LAUNCH(wz_k_splitk_reduce_group, dim3(g.first[g.n]), dim3(256), 0, s, g);
}

void wz_launch_splitk_reduce(const WzConvArgs& a, const float* ws, hipStream_t s) {
    const int total = a.M * (a.n_pad >> 2);
    WZ_LAUNCH(wz_k_splitk_reduce, dim3((total + 255) / 256), dim3(256), 0, s, a, ws);
}

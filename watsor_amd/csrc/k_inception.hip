// SSD-Inception-v2 (watsor_amd/inception.py): the ops MobileNet-v2 does not have.
//
//  wz_k_stem7      fp16 engine: Conv2d_1a_7x7 (the separable stem folded into one dense 7x7x3x64 kernel by the builder), stride 2, on the
//                  4-channel fp16 network input, + bias, relu6.  Implicit GEMM on v_mfma_f32_16x16x32_f16 with K packed as tap * 4 + c:
//                  49 taps x 4 input halves = 196 -> 7 chunks of 32, so a lane group's 8 K values are the 4-channel pixels of two taps,
//                  two 8-byte loads as they lie in the input tensor (the split-operand stem block packs its K the same way).  A generic
//                  conv would spend one 32-wide chunk per tap: 49 chunks, ~87 % of the MFMA work on zeros.  A wave holds the whole
//                  64 x 224 weight matrix in registers (7 chunks x 4 channel tiles of A fragments) and walks 16-pixel tiles.
//  wz_k_stem7_f32  fp32 engine: the same conv as a direct loop (weights in LDS, 8 output channels per thread), reading the input as a
//                  hi + lo pair like wz_k_stem_f32.
//  wz_k_pool3      3x3 max / average pool, stride 1 or 2, TF 'SAME', half or float; a thread owns 16 bytes of channels of one output
//                  pixel.  Max ignores the padding; average divides the sum of the in-image taps by their number (TF's AvgPool).
//
// Every kernel here writes channels [coff, coff + C) of an output tensor with cstride channels per pixel: an Inception module's
// branches write their slices of the concat, no copy.
#include "wz_common.h"

#define WZ_STEM7_KC 7          // 32-row K chunks: taps 0 .. 55 (49 .. 55 zero) x 4 channels
#define WZ_STEM7_COUT 64
#define WZ_STEM7_TILES_PER_WAVE 4

__global__ __launch_bounds__(256) void wz_k_stem7(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                                  const float* __restrict__ bias, half_t* __restrict__ out, int M, int hin, int win,
                                                  int hout, int wout, int pad_t, int pad_l, int cstride, int coff) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    // A fragments: lane l of channel tile nt, chunk c holds W[k = c * 32 + g * 8 + j][n = nt * 16 + r16] (engine.pack_conv_weights, 1 tap)
    half8_t wf[WZ_STEM7_KC][4];
#pragma unroll
    for (int c = 0; c < WZ_STEM7_KC; ++c)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) wf[c][nt] = *reinterpret_cast<const half8_t*>(w + ((size_t)(nt * WZ_STEM7_KC + c) * 64 + lane) * 8);
    float4_t bv[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) bv[nt] = *reinterpret_cast<const float4_t*>(bias + nt * 16 + g * 4);
    const int hw = hout * wout;
    const int tiles = (M + 15) >> 4;
    const half4_t zero4 = {0, 0, 0, 0};
    for (int tile = blockIdx.x * 4 + wave; tile < tiles; tile += gridDim.x * 4) {
        const int m = tile * 16 + r16;
        const bool mv = m < M;
        const int mm = mv ? m : 0;
        const int b = mm / hw, rem = mm - b * hw;
        const int oy = rem / wout, ox = rem - oy * wout;
        const int iy0 = oy * 2 - pad_t, ix0 = ox * 2 - pad_l;
        const half_t* inb = in + (size_t)b * hin * win * 4;
        float4_t acc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < WZ_STEM7_KC; ++c) {
            half8_t x;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int t = c * 8 + g * 2 + j;           // this lane group's two taps of the chunk
                const int ky = t / 7, kx = t - ky * 7;
                const int iy = iy0 + ky, ix = ix0 + kx;
                const bool ok = mv && t < 49 && iy >= 0 && iy < hin && ix >= 0 && ix < win;
                const half4_t p = ok ? *reinterpret_cast<const half4_t*>(inb + ((size_t)iy * win + ix) * 4) : zero4;
                x[j * 4 + 0] = p[0];
                x[j * 4 + 1] = p[1];
                x[j * 4 + 2] = p[2];
                x[j * 4 + 3] = (half_t)0;                   // (the input's fourth channel meets zero weights; keep it out of the sum)
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[c][nt], x, acc[nt], 0, 0, 0);
        }
        // D layout: lane holds channels nt * 16 + g * 4 .. + 3 of pixel r16
        if (mv) {
            half_t* o = out + (size_t)m * cstride + coff + g * 4;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) *reinterpret_cast<half4_t*>(o + nt * 16) = wz_relu6_pack(acc[nt], bv[nt], true);
        }
    }
}

void wz_launch_stem7(const half_t* in, const half_t* w, const float* bias, half_t* out, int n, int hin, int win, int hout, int wout,
                     int pad_t, int pad_l, int cstride, int coff, hipStream_t s) {
    const int M = n * hout * wout;
    const int tiles = (M + 15) / 16;
    const int grid = (tiles + 4 * WZ_STEM7_TILES_PER_WAVE - 1) / (4 * WZ_STEM7_TILES_PER_WAVE);
    WZ_LAUNCH(wz_k_stem7, dim3(grid), dim3(256), 0, s, in, w, bias, out, M, hin, win, hout, wout, pad_t, pad_l, cstride, coff);
}

__global__ __launch_bounds__(256) void wz_k_stem7_f32(const half_t* __restrict__ in, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int total, int hin,
                                                      int win, int hout, int wout, int pad_t, int pad_l, int pair, int cstride, int coff) {
    __shared__ float sw[49 * 3 * WZ_STEM7_COUT + WZ_STEM7_COUT];
    for (int i = threadIdx.x; i < 49 * 3 * WZ_STEM7_COUT; i += 256) sw[i] = w[i];
    if (threadIdx.x < WZ_STEM7_COUT) sw[49 * 3 * WZ_STEM7_COUT + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= total) return;
    const int cg = tid & 7, pix = tid >> 3;             // 8 output channels of one pixel
    const int ox = pix % wout;
    const int t2 = pix / wout;
    const int oy = t2 % hout, b = t2 / hout;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = sw[49 * 3 * WZ_STEM7_COUT + cg * 8 + j];
    for (int ky = 0; ky < 7; ++ky) {
        const int iy = oy * 2 - pad_t + ky;
        if (iy < 0 || iy >= hin) continue;
        for (int kx = 0; kx < 7; ++kx) {
            const int ix = ox * 2 - pad_l + kx;
            if (ix < 0 || ix >= win) continue;
            const size_t px = (size_t)(b * hin + iy) * win + ix;
            const half4_t p = *reinterpret_cast<const half4_t*>(in + px * (pair ? 8 : 4));
            half4_t pl = {0, 0, 0, 0};
            if (pair) pl = *reinterpret_cast<const half4_t*>(in + px * 8 + 4);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = (float)p[c] + (float)pl[c];
                const float* wr = sw + ((ky * 7 + kx) * 3 + c) * WZ_STEM7_COUT + cg * 8;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(x, wr[j], acc[j]);
            }
        }
    }
    float4_t o0, o1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o0[j] = fminf(fmaxf(acc[j], 0.0f), 6.0f);
        o1[j] = fminf(fmaxf(acc[4 + j], 0.0f), 6.0f);
    }
    float* o = out + (size_t)pix * cstride + coff + cg * 8;
    *reinterpret_cast<float4_t*>(o) = o0;
    *reinterpret_cast<float4_t*>(o + 4) = o1;
}

void wz_launch_stem7_f32(const half_t* in, const float* w, const float* bias, float* out, int n, int hin, int win, int hout, int wout,
                         int pad_t, int pad_l, int cstride, int coff, bool pair, hipStream_t s) {
    const int total = n * hout * wout * (WZ_STEM7_COUT / 8);
    WZ_LAUNCH(wz_k_stem7_f32, dim3((total + 255) / 256), dim3(256), 0, s, in, w, bias, out, total, hin, win, hout, wout, pad_t, pad_l,
              pair ? 1 : 0, cstride, coff);
}

// 16 bytes of channels: 8 halves or 4 floats
template <typename T> struct WzVec;
template <> struct WzVec<half_t> { typedef half8_t type; enum { N = 8 }; };
template <> struct WzVec<float> { typedef float4_t type; enum { N = 4 }; };

template <typename T>
__global__ __launch_bounds__(256) void wz_k_pool3(const T* __restrict__ in, T* __restrict__ out, int total, int hin, int win, int c,
                                                  int hout, int wout, int stride, int pad_t, int pad_l, int is_max, int cstride, int coff) {
    typedef typename WzVec<T>::type V;
    constexpr int N = WzVec<T>::N;
    const int tid = blockIdx.x * 256 + threadIdx.x;
    if (tid >= total) return;
    const int cv = c / N;
    const int cg = tid % cv, pix = tid / cv;
    const int ox = pix % wout;
    const int t2 = pix / wout;
    const int oy = t2 % hout, b = t2 / hout;
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = is_max ? -INFINITY : 0.0f;
    int taps = 0;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - pad_t + ky;
        if (iy < 0 || iy >= hin) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - pad_l + kx;
            if (ix < 0 || ix >= win) continue;
            const V x = *reinterpret_cast<const V*>(in + ((size_t)(b * hin + iy) * win + ix) * c + cg * N);
            ++taps;
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = is_max ? fmaxf(acc[j], (float)x[j]) : acc[j] + (float)x[j];
        }
    }
    V o;
    const float inv = is_max ? 1.0f : 1.0f / (float)taps;   // (SAME padding leaves every output pixel at least one in-image tap)
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = (T)(is_max ? acc[j] : acc[j] * inv);
    *reinterpret_cast<V*>(out + (size_t)pix * cstride + coff + cg * N) = o;
}

template <typename T>
static void wz_launch_pool3_t(const T* in, T* out, int n, int hin, int win, int c, int hout, int wout, int stride, int pad_t, int pad_l,
                              bool is_max, int cstride, int coff, hipStream_t s) {
    const int total = n * hout * wout * (c / WzVec<T>::N);
    WZ_LAUNCH(wz_k_pool3<T>, dim3((total + 255) / 256), dim3(256), 0, s, in, out, total, hin, win, c, hout, wout, stride, pad_t, pad_l,
              is_max ? 1 : 0, cstride, coff);
}

void wz_launch_pool3(const half_t* in, half_t* out, int n, int hin, int win, int c, int hout, int wout, int stride, int pad_t, int pad_l,
                     bool is_max, int cstride, int coff, hipStream_t s) {
    wz_launch_pool3_t<half_t>(in, out, n, hin, win, c, hout, wout, stride, pad_t, pad_l, is_max, cstride, coff, s);
}

void wz_launch_pool3_f32(const float* in, float* out, int n, int hin, int win, int c, int hout, int wout, int stride, int pad_t, int pad_l,
                         bool is_max, int cstride, int coff, hipStream_t s) {
    wz_launch_pool3_t<float>(in, out, n, hin, win, c, hout, wout, stride, pad_t, pad_l, is_max, cstride, coff, s);
}

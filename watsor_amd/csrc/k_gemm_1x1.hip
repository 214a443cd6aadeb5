// Conv_1 (1x1, 320 -> 1 280 on the 10x10 map) as what it is: a dense GEMM, D[n][m] = sum_k W[n][k] X[m][k], M = frames x 100 pixels.
//
// Why not the convolution kernels.  wz_k_conv_ws (k_conv.hip) gives a workgroup 32 pixels x 64 channels, cuts K four ways over its waves and has
// every wave pull its own activation AND weight fragments out of L2: (32 + 64) x 640 x 2 B = 123 KB per workgroup, 61 MB per batch of eight for
// 2.1 MB of operands, plus 32 KiB of LDS and a barrier to add the four K slices up, plus two integer divisions per pixel tile and wave to find a
// (frame, row, column) that a 1x1 stride-1 convolution never needs.  Here:
//   * a workgroup = WZ_G1_TM pixels x 128 channels, four waves of WZ_G1_TM x 32 each.  A wave owns its channels outright: it walks ALL of K for
//     them (no K slices, no partial sums, no reduction) and loads their weight fragments straight from L2 into registers -- the packed layout is
//     fragment order and no other wave needs them (as in k_conv_wide.hip);
//   * the pixel tile is fetched ONCE per workgroup, in whole 128-byte lines, and shared through LDS: pixel m is row m of the source tensor, at
//     m * cin halves (no divisions), read through a buffer descriptor that ends with the tensor, so the rows of a part-filled last tile read
//     zeros.  All of K is staged at once (WZ_G1_STEPS steps of 64 channels: 20 KiB for 32 pixels x 320 channels) in k_conv_wide.hip's image: one
//     [pixel][128 B] slab per step, the 16-byte slot of a pixel's row XOR-swizzled by (pixel >> 1) & 7 -- lane-linear writes, conflict-free
//     fragment reads;
//   * one memory round trip and a bit: every activation load of the wave and its first weight groups are issued before anything waits for them;
//     the remaining weight groups are requested behind the barrier and arrive under the first MFMAs.
// DUP: the source tensor holds its fp16 values TWICE per pixel ([x | x], WZ_OPF_DUP_OUT of the block in front: the robust program) and the packed
// weights have K = 2 * 320, hi halves over the first copy, lo halves over the second.  W_hi x + W_lo x needs x once: only the first cin / 2
// channels of a row are staged (the row pitch stays cin) and every activation fragment is multiplied with weight chunk c and with chunk c + kc / 2.
// The engine sets WzConvArgs::dup_k from the producing op's flag; nothing is inferred from shapes.
// The K order of an output is fixed -- step, chunk of the step, hi then lo -- whatever the pixel's place in a tile or a batch: a frame's rows do
// not depend on the frames around it.  Epilogue: wz_epilogue4, as every fp16 convolution.
#include "wz_common.h"

typedef __attribute__((ext_vector_type(4))) unsigned int uint4_t;

// 32 x 128 workgroup tiles (250 workgroups at batch 8, 124 registers, 20 KiB of LDS, four workgroups per CU).  64 x 128 (130 workgroups, 144 registers,
// 40 KiB) was built and measured beside it and lost on the kernel's own time -- batch 8 alone 6.5 us against 5.2 us (the older kernel: 8.6 us), under
// load 11.5 against 10.8 us -- with frames/s equal within their spread: a wave's 160 MFMAs are a longer chain than its 80 here, and that chain is what
// a launch this short lasts (profiles/gemm_1x1_kernel_stats_lanes1.txt, profiles/gemm_1x1_lane_overlap.txt).
#define WZ_G1_TM 32      // pixels per workgroup
#define WZ_G1_TN 128     // channels per workgroup: four waves x two 16-channel tiles
#define WZ_G1_STEPS 5    // 64-channel K steps: the staged K is 320 channels, all of it in the LDS image at once (straight-line code, no step loop)
// Measured alone (HIP events, 8 launches per bracket; profiles/gemm_1x1_kernel_stats_lanes1.txt), this kernel against what served Conv_1 before:
//   robust program (K = 2 x 320):  100 pixels 4.8 against 4.1 us, 200: 4.8 / 5.5, 300: 4.8 / 5.7, 400: 4.9 / 7.6, 800: 5.2 / 8.6, 1 600: 7.0 / 12.2
//   default program (K = 320):     100 pixels 3.7 against 3.5 us, 200: 3.8 / 7.4, 300: 3.8 / 7.3, 400: 3.8 / 7.3, 800: 4.0 / 7.4
// One frame stays where it was (160 workgroups that cut K eight ways finish sooner than 40 that walk it alone); from two frames on this one wins.
#define WZ_G1_MIN_M 200  // pixels from which the launch takes this kernel

template <bool DUP>
__global__ __launch_bounds__(256, 2) void wz_k_gemm_1x1(const WzConvArgs a) {
    WZ_LANE_STAMP(a.dbg);
    constexpr int TM = WZ_G1_TM, MT = TM / 16, NT = 2, S = WZ_G1_STEPS, NF = DUP ? 2 : 1, XI = TM / 32;
    constexpr int PRE = DUP ? 3 : S;   // steps whose weights are requested with the activations (the others: behind the barrier)
    __shared__ __attribute__((aligned(16))) unsigned char smem[S * TM * 128];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    int bx, by;
    {   // XCD-aware tile order (as k_conv_wide.hip): an XCD's workgroups are neighbours in (pixel tile, channel group) order and share weight slices in its L2
        const int L = (int)blockIdx.x, total = a.grid_m * a.grid_n;
        const int xcd = L & 7, slot = L >> 3;
        const int qd = total >> 3, rm = total & 7;
        const int V = (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + slot;
        bx = V % a.grid_m;
        by = V / a.grid_m;
    }
    const int m_base = bx * TM;
    const int nt_w = by * (WZ_G1_TN / 16) + wave * NT;   // the wave's first 16-channel tile
    const int kcw = a.kc;                                // weight chunks (32 channels) per tile

    // activations: instruction i of this wave = pixels i*32 + wave*8 + (lane >> 3), 16-byte chunk (lane & 7) ^ swizzle of the step's 128 bytes
    const unsigned row = (unsigned)a.cin * 2u;
    const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc((void*)a.in, 0, (int)((unsigned)a.M * row), 0x00020000);
    const unsigned chunk = (unsigned)((lane & 7) ^ ((wave * 4 + (lane >> 4)) & 7));
    uint4_t rb[S][XI];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const unsigned m = (unsigned)(m_base + i * 32 + wave * 8 + (lane >> 3));   // (a row at or past M lies beyond the descriptor: zeros)
            rb[s][i] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, m * row + chunk * 16u, s * 128, 0);
        }

    // weights: fragment (tile, chunk) = 1 KiB at (tile * kc + chunk) * 1 KiB, the lane's 16 bytes of it
    const half_t* const wl = a.w + (size_t)nt_w * kcw * 512 + lane * 8;
    half8_t wf[S][2][NT][NF];
    auto load_w = [&](int s) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    wf[s][h][nt][f] = *reinterpret_cast<const half8_t*>(wl + ((size_t)nt * kcw + (s * 2 + h) + f * (kcw >> 1)) * 512);
    };
#pragma unroll
    for (int s = 0; s < PRE; ++s) load_w(s);

    float4_t acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (float4_t){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int i = 0; i < XI; ++i)
            *reinterpret_cast<uint4_t*>(smem + s * (TM * 128) + (i * 32 + wave * 8) * 128 + lane * 16) = rb[s][i];
    __syncthreads();
#pragma unroll
    for (int s = PRE; s < S; ++s) load_w(s);

#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            half8_t xa[MT];   // pixel P = mt*16 + r16, chunk h*4 + g of the step, slot swizzled by (P >> 1) & 7
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                xa[mt] = *reinterpret_cast<const half8_t*>(smem + s * (TM * 128) + (mt * 16 + r16) * 128 + (((h * 4 + g) ^ ((r16 >> 1) & 7)) * 16));
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s][h][nt][f], xa[mt], acc[mt][nt], 0, 0, 0);
        }
    }

    // D layout: lane holds rows (n) g*4 .. g*4+3 of column (m) r16
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) wz_epilogue4(a, m_base + mt * 16 + r16, (nt_w + nt) * 16 + g * 4, acc[mt][nt]);
}

// A 1x1 stride-1 unpadded convolution into an activation tensor, whole 128-channel workgroup tiles, a staged K of exactly WZ_G1_STEPS 64-channel
// steps, and a source small enough for a 32-bit descriptor.  Of those, the shapes this kernel was measured on and wins: Conv_1's
// (K = 320, N = 1 280; profiles/gemm_1x1_*.txt).  A pure function of the shape: a batch's rows never depend on what else is in flight.
bool wz_gemm_1x1_applies(const WzConvArgs& a) {
    const int kstaged = a.dup_k ? a.kc >> 1 : a.kc;   // 32-channel chunks
    return a.out_mode == WZ_OUT_ACT && a.ksize == 1 && a.stride == 1 && a.pad_t == 0 && a.pad_l == 0 && a.hin == a.hout && a.win == a.wout &&
           a.cin == a.kc * 32 && (!a.dup_k || a.kc % 2 == 0) && kstaged == 2 * WZ_G1_STEPS &&
           a.n_pad >= 1024 && a.n_pad % WZ_G1_TN == 0 && a.M >= WZ_G1_MIN_M && (long long)(a.M + WZ_G1_TM) * a.cin * 2 < (1ll << 31);
}

void wz_launch_gemm_1x1(const WzConvArgs& a0, hipStream_t s) {
    WzConvArgs a = a0;
    a.grid_m = (a.M + WZ_G1_TM - 1) / WZ_G1_TM;
    a.grid_n = a.n_pad / WZ_G1_TN;
    const dim3 grid(a.grid_m * a.grid_n);
    if (a.dup_k)
        WZ_LAUNCH(wz_k_gemm_1x1<true>, grid, dim3(256), 0, s, a);
    else
        WZ_LAUNCH(wz_k_gemm_1x1<false>, grid, dim3(256), 0, s, a);
}

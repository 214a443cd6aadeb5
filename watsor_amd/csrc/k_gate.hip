// Gated tiled detection (include/watsor_hip.h: wz_set_camera_tiles / wz_detect_gated): the two launches around the
// host's decision which tiles of a camera run.
//   wz_k_tile_activity  every tile of a call in one launch: the lumas of each cell of WZ_GATE_CELL x WZ_GATE_CELL pixels are summed (the
//                       tile's new grid, uint16 a cell) and compared with the tile's reference grid; the number of cells that moved by
//                       more than pixel_thr a pixel is the tile's activity, which the host reads from page-locked memory.
//   wz_k_gate_commit    behind the batch: a tile that ran gets its new grid as reference and its fresh rows as cached rows; fresh or
//                       cached, every tile's rows go into one block, in tile order, for wz_k_merge_tiles.
// Integer sums only: any order of summation gives the same bytes (tests/gate_oracle.py restates them with numpy).
// A tile with an ignore mask (WzGateTile::ignore) runs wz_k_tile_activity<true>: a changed cell whose mask bit is set
// is not counted; the sums are the same.  A launch none of whose tiles has a mask runs <false>, the kernel there was before there was one.
#include "wz_common.h"

#define WZ_GATE_THREADS 1024   // 16 waves: one wave per pixel row of a strip of cells

__device__ __forceinline__ uint32_t wz_gate_byte(const uint4& v, int j) {
    const uint32_t w = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 255u;
}

// One workgroup per strip of cells (grid.x) of a tile (grid.y); one wave per pixel row of the strip.  A wave walks its row in aligned
// 16-byte words, 64 at a time: lane l owns word base + l -- one 16-byte load where the word lies inside the row, byte loads at the row's two
// ragged ends, no byte outside [row, row + row_bytes) and every byte once (the next 64 words are in flight while these are summed).  A word
// is no wider than a cell's bytes in a row (16, 32 or 48), so its lumas fall into at most two cells: two LDS adds per lane.  A 3-byte pixel
// that straddles two words is finished by the lane that holds its last byte: the weighted sum of its first bytes comes from the lane
// before (a shuffle; lane 0 takes it from lane 63 of the wave's previous step along the row).
template <bool MASK>
__global__ __launch_bounds__(WZ_GATE_THREADS) void wz_k_tile_activity(const WzGateTile* __restrict__ tiles, int32_t* counters,
                                                                      int32_t* __restrict__ activity) {
    extern __shared__ uint32_t wz_gate_cells[];   // [cols of the widest tile of the launch]
    __shared__ int changed;
    const WzGateTile t = tiles[blockIdx.y];
    const int strip = blockIdx.x, tid = threadIdx.x;
    if (strip >= t.crows) return;
    for (int c = tid; c < t.cols; c += WZ_GATE_THREADS) wz_gate_cells[c] = 0;
    if (tid == 0) changed = 0;
    __syncthreads();

    const int lane = tid & 63, row = strip * WZ_GATE_CELL + (tid >> 6);
    if (row < t.th) {
        const uint8_t* rs = t.src + (size_t)row * (size_t)t.pitch;
        const int head = (int)(reinterpret_cast<uintptr_t>(rs) & 15u), rb = t.row_bytes;
        const int words = (head + rb + 15) >> 4;
        const int mode = t.mode;
        const int cell_shift = mode == WZ_GATE_GRAY ? 4 : 5;   // bytes of a cell in a row: 16, 32 (4:2:2) -- or 48 (three bytes a pixel)
        const bool three = mode == WZ_GATE_RGB || mode == WZ_GATE_BGR;
        const uint32_t w_first = mode == WZ_GATE_RGB ? 77u : 29u, w_last = mode == WZ_GATE_RGB ? 29u : 77u;
        auto load = [&](int k) -> uint4 {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (k >= words) return v;
            const int lo = k * 16 - head;
            if (lo >= 0 && lo + 16 <= rb) return *reinterpret_cast<const uint4*>(rs + lo);
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int o = lo + j;
                if (o >= 0 && o < rb) w[j >> 2] |= (uint32_t)rs[o] << (8 * (j & 3));
            }
            return make_uint4(w[0], w[1], w[2], w[3]);
        };
        uint32_t carry63 = 0;   // three bytes a pixel: what lane 63 of the previous step left of a pixel that ends in this step's first word
        uint4 nxt = load(lane);
        for (int base = 0; base < words; base += 64) {
            const uint4 v = nxt;
            const int k = base + lane;
            if (base + 64 < words) nxt = load(k + 64);
            const int lo = k * 16 - head;              // the word's first byte, counted from the row's first (negative in the row's first word)
            const int lo0 = lo < 0 ? 0 : lo;
            uint32_t sum_a = 0, sum_b = 0;
            int cell_a, bnd;                           // bytes j < bnd of the word belong to cell_a, the others to cell_a + 1
            if (!three) {
                cell_a = lo0 >> cell_shift;
                bnd = ((cell_a + 1) << cell_shift) - lo;
                // which bytes are lumas: all of them, or those whose offset in the row is even (YUYV) / odd (UYVY)
                // WZ_GATE_LOW10: the luma of a word lo | hi << 8 is bits 2 .. 9 = (lo >> 2) + ((hi & 3) << 6) -- a sum over its two bytes, which lie
                // in one cell (a cell's 32 bytes start at an even offset) though not always in one 16-byte word: each byte adds its share
                const bool low10 = mode == WZ_GATE_LOW10;
                const int sel = mode == WZ_GATE_GRAY ? -1 : (((mode == WZ_GATE_UYVY) ? 1 : 0) ^ (head & 1));
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t raw = wz_gate_byte(v, j);
                    const uint32_t b = low10 ? (((j ^ head) & 1) ? (raw & 3u) << 6 : raw >> 2) : (sel < 0 || (j & 1) == sel) ? raw : 0u;
                    sum_a += j < bnd ? b : 0u;
                    sum_b += j < bnd ? 0u : b;
                }
            } else {
                cell_a = lo0 / 48;
                bnd = (cell_a + 1) * 48 - lo;
                const int m = (lo + 48) % 3;           // channel of the word's byte 0 (the row begins with a pixel; lo >= -15)
                const int e = (5 - m) % 3;             // the word's first byte that ends a pixel: 0, 1 or 2
                // weights of bytes j = 0, 1, 2 (mod 3) of the word; bytes outside the row are zero and add nothing
                uint32_t wr[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int ch = (m + i) % 3;
                    wr[i] = ch == 0 ? w_first : ch == 1 ? 150u : w_last;
                }
                // what this word holds of a pixel that ends in the next word: bytes 14, 15 (e == 1), byte 15 (e == 2), nothing (e == 0)
                const uint32_t tail = e == 0 ? 0u : (e == 1 ? wr[2] * wz_gate_byte(v, 14) : 0u) + wr[0] * wz_gate_byte(v, 15);
                uint32_t acc = __shfl_up(tail, 1);
                if (lane == 0) acc = carry63;
                carry63 = __shfl(tail, 63);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    acc += wr[j % 3] * wz_gate_byte(v, j);
                    if (j % 3 == e) {                  // a pixel ends here (outside the row: acc == 0, luma 0)
                        const uint32_t luma = (acc + 128u) >> 8;
                        sum_a += j < bnd ? luma : 0u;
                        sum_b += j < bnd ? 0u : luma;
                        acc = 0;
                    }
                }
            }
            if (k < words) {
                if (sum_a) atomicAdd(&wz_gate_cells[cell_a], sum_a);
                if (sum_b && cell_a + 1 < t.cols) atomicAdd(&wz_gate_cells[cell_a + 1], sum_b);
            }
        }
    }
    __syncthreads();

    const int ch = min(WZ_GATE_CELL, t.th - strip * WZ_GATE_CELL);
    for (int c = tid; c < t.cols; c += WZ_GATE_THREADS) {
        const uint32_t s = wz_gate_cells[c];
        const size_t at = (size_t)strip * t.cols + c;
        t.now[at] = (uint16_t)s;
        if (t.ref) {
            const int cw = min(WZ_GATE_CELL, t.tw - c * WZ_GATE_CELL);
            const int d = (int)s - (int)t.ref[at];
            if ((d < 0 ? -d : d) > t.thr * cw * ch && !(MASK && t.ignore && ((t.ignore[at >> 5] >> (at & 31)) & 1u))) atomicAdd(&changed, 1);
        }
    }
    __syncthreads();
    // the tile's count: every strip adds its own, the strip that arrives last hands the sum to the host and leaves both counters zero
    if (tid == 0) {
        int32_t* cnt = counters + 2 * blockIdx.y;
        if (changed) atomicAdd(&cnt[0], changed);
        __threadfence();
        if (atomicAdd(&cnt[1], 1) == t.crows - 1) {
            __threadfence();
            activity[blockIdx.y] = atomicExch(&cnt[0], 0);
            atomicExch(&cnt[1], 0);
        }
    }
}

void wz_launch_tile_activity(const WzGateTile* tiles, int n, int max_crows, int max_cols, int32_t* counters, int32_t* activity, hipStream_t s,
                             bool with_mask) {
    const auto kernel = with_mask ? wz_k_tile_activity<true> : wz_k_tile_activity<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)max_crows, (unsigned)n), dim3(WZ_GATE_THREADS), (size_t)max_cols * 4, s, tiles, counters,
                       activity);
}

// One workgroup per tile of the call.  Rows are 72 bytes, a tile's 100 of them 450 16-byte words; every block of rows is 16-byte aligned.
__global__ __launch_bounds__(256) void wz_k_gate_commit(const WzGateCommit* __restrict__ tiles, const wz_detection_t* batch_rows, wz_detection_t* out) {
    static_assert(sizeof(wz_detection_t) * WZ_MAX_DETECTIONS % 16 == 0, "a tile's rows are whole 16-byte words");
    constexpr int WORDS = (int)(sizeof(wz_detection_t) * WZ_MAX_DETECTIONS / 16);
    const WzGateCommit t = tiles[blockIdx.x];
    const int tid = threadIdx.x;
    uint4* dst = reinterpret_cast<uint4*>(out + (size_t)blockIdx.x * WZ_MAX_DETECTIONS);
    uint4* cache = reinterpret_cast<uint4*>(t.cache);
    if (t.fresh < 0) {
        for (int i = tid; i < WORDS; i += 256) dst[i] = cache[i];
        return;
    }
    const uint4* src = reinterpret_cast<const uint4*>(batch_rows + (size_t)t.fresh * WZ_MAX_DETECTIONS);
    for (int i = tid; i < WORDS; i += 256) {
        const uint4 v = src[i];
        dst[i] = v;
        cache[i] = v;
    }
    for (int i = tid; i < t.cells; i += 256) t.ref[i] = t.now[i];
}

void wz_launch_gate_commit(const WzGateCommit* tiles, int n, const wz_detection_t* batch_rows, wz_detection_t* out, hipStream_t s) {
    hipLaunchKernelGGL(wz_k_gate_commit, dim3((unsigned)n), dim3(256), 0, s, tiles, batch_rows, out);
}

// Motion regions (include/watsor_hip.h: wz_set_camera_motion / wz_detect_motion): the launch between the whole-frame
// activity launch (k_gate.hip) and the host's read of the rectangles.
//   wz_k_motion_regions  one workgroup per camera of the call.  The grid of 16 x 16-pixel luma sums against the previous call's grid gives
//                        the changed cells C; C dilated gives D; the 8-connected components of D are labelled in LDS; a component's weight
//                        n is its number of C cells; the 64 heaviest components with n >= min_cells are ranked; one wave walks them and
//                        writes at most WZ_MOTION_MAX_REGIONS rectangles into the lane's page-locked block.
//   wz_k_motion_still    behind the merge of a motion call: a frame without a tile gets the padding rows and pass bytes 0.
//   wz_k_motion_stamp    last of a motion call with a camera that holds under detections: the cells under every
//                        passing row are raised to object_hold in the camera's age grid.
// A camera with a hold (WzMotionCam::age_out) runs wz_k_motion_regions<true>: step 1 reads the cell's age beside its two sums, votes
// "changed or age > 0" into the bit map and writes the decayed age; everything behind step 1 reads the bit map and is the same code.  A
// camera without one takes, in either instantiation, the path it always took.
// A camera with an ignore mask (WzMotionCam::ignore) runs wz_k_motion_regions<.., true>: step 1 reads the wave's 64
// mask bits -- one aligned 64-bit word, the same address in every lane -- beside its loads and clears the ignored lanes of `changed` before
// the vote, the age write and the popcounts; what the mask removed is counted into WzMotionOut::ignored.  Four instantiations; a launch
// none of whose cameras has a mask runs <false, false> or <true, false>, which are the two kernels there were before there was a mask.
// Integers only.  Nothing depends on scheduling: a component's id is the SMALLEST linear index of its cells, ties in n are broken by id,
// sums and minima may be taken in any order (tests/motion_oracle.py restates all of it with numpy).
//
// Labelling: label equivalence with pointer jumping.  Every D cell starts as its own root (label = its index; a label is always the index
// of a cell of the same component, and label[r] <= r).  A round is
//   scan      a cell whose 3 x 3 neighbourhood holds a label m below its own label l links l's tree under m: label[l] = min(label[l], m)
//   compress  every cell follows label[] to its root and takes the root as its label
// until a round links nothing (a flag in LDS, read by every thread behind a barrier).  Every round that sets the flag lowers the label of
// the cell that set it, so the loop ends; when it ends every cell's label is no larger than its neighbours', i.e. constant on a component,
// and the component's smallest cell can only point at itself: the label is the smallest index.  Trees merge whole, so the number of rounds
// grows with the logarithm of a component's longest path, not with the path (a one-cell serpentine over a 1080p grid is 4047 sweeps of a
// plain 3 x 3 minimum).
#include <limits.h>
#include <stddef.h>

#include "wz_common.h"

#define WZ_MOTION_BG 0xffffu       // label of a cell outside D (cell indices stay below WZ_MOTION_MAX_CELLS = 32768)
#define WZ_MOTION_RANKED 0xffc0u     // a root's count replaced by 0xffc0 | rank (a count is at most 32768)
#define WZ_MOTION_NEAR_KEYS 2048    // components ranked by counting in LDS; beyond that, by repeated selection
static_assert(WZ_MOTION_MAX_CELLS <= 32768, "labels are uint16, keys hold 15 bits of id and 16 of n");
static_assert(WZ_MOTION_CANDIDATES == 64, "a candidate's rank is stored in 6 bits");

// label[i] = min(label[i], v) on a uint16 in LDS: compare-and-swap on the 32-bit word that holds it
__device__ __forceinline__ void wz_motion_min16(uint16_t* labels, uint32_t i, uint32_t v) {
    uint32_t* wp = reinterpret_cast<uint32_t*>(labels) + (i >> 1);
    const uint32_t sh = (i & 1u) * 16u;
    uint32_t old = *reinterpret_cast<volatile uint32_t*>(wp);
    for (;;) {
        if (((old >> sh) & 0xffffu) <= v) return;
        const uint32_t want = (old & ~(0xffffu << sh)) | (v << sh);
        const uint32_t seen = atomicCAS(wp, old, want);
        if (seen == old) return;
        old = seen;
    }
}
// a word other threads of the workgroup wrote or added to in device memory (read at the L2, not from this CU's cache)
__device__ __forceinline__ uint32_t wz_motion_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one axis of the walk: [a0, a1) grown evenly to `side` pixels, shifted back into [0, size), then cut at even pixels where the format asks
__device__ __forceinline__ void wz_motion_axis(int& a0, int& a1, int size, int min_side, int even) {
    const int m = min(min_side, size), d = m - (a1 - a0);
    if (d > 0) {
        a0 -= d / 2;
        a1 += d - d / 2;
        if (a0 < 0) a1 -= a0, a0 = 0;
        if (a1 > size) a0 -= a1 - size, a1 = size;
    }
    if (even) {
        a0 &= ~1;
        a1 = min(size, (a1 + 1) & ~1);
    }
}

// A thread's cells i0, i0 + WZ_MOTION_THREADS, ... with their column and row: one division, then additions
struct WzMotionWalk {
    int i, x, y, gw, dx, dy;
    __device__ __forceinline__ WzMotionWalk(int i0, int gw_) : i(i0), gw(gw_) {
        y = i0 / gw_; x = i0 - y * gw_;
        dy = WZ_MOTION_THREADS / gw_; dx = WZ_MOTION_THREADS - dy * gw_;
    }
    __device__ __forceinline__ void next() {
        i += WZ_MOTION_THREADS; x += dx; y += dy;
        if (x >= gw) x -= gw, ++y;
    }
};

// AGE: the launch has a camera with a hold.  `aged`, below, is this workgroup's camera having one; "changed" then reads "active" in every
// comment behind step 1.  The ages go from device memory to device memory: none of them is ever in LDS.
// MASK: the launch has a camera with an ignore mask; a camera of it without one reads no mask word.
template <bool AGE, bool MASK>
__global__ __launch_bounds__(WZ_MOTION_THREADS) void wz_k_motion_regions(const WzMotionCam* __restrict__ cams, WzMotionOut* __restrict__ outs) {
    // C, one bit a cell: 2 * ceil(cells / 64) words; the labels, uint16 a cell; the counts, uint16 a cell (a component's n, at its root)
    extern __shared__ uint32_t wz_motion_lds[];
    __shared__ int again, row_lo, row_hi;   // row_lo .. row_hi: the rows of cells that hold a changed cell
    __shared__ uint32_t n_keys;
    __shared__ uint32_t n_active, n_held;   // (AGE) the popcounts of step 1's votes: active cells, and those of them that did not change
    __shared__ uint32_t n_ignored;          // (MASK) the changed cells that the mask removed
    __shared__ uint32_t near_keys[WZ_MOTION_NEAR_KEYS];   // the first keys found, where ranking by counting reads them
    __shared__ uint32_t cand_key[WZ_MOTION_CANDIDATES];   // the ranked keys: n << 15 | (32767 - id)
    __shared__ int32_t box[WZ_MOTION_CANDIDATES][4];      // their cell boxes: cx0, cx1, cy0, cy1
    __shared__ WzMotionOut result;
    constexpr int RESULT_WORDS = (int)(sizeof(WzMotionOut) / 4), IGNORED_WORD = (int)(offsetof(WzMotionOut, ignored) / 4);

    const WzMotionCam c = cams[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t* const out_words = reinterpret_cast<uint32_t*>(outs + blockIdx.x);
    const bool aged = AGE && c.age_out != nullptr;
    if (!c.ref && !aged) {   // no reference: nothing has changed (the same for every thread of the workgroup)
        if (tid < RESULT_WORDS) out_words[tid] = 0u;
        return;
    }
    const int gw = c.gw, cells = c.gw * c.gh;
    const int cwords = ((cells + 63) >> 6) * 2, lwords = (cells + 1) >> 1;
    const int span = (cells + WZ_MOTION_THREADS - 1) & ~(WZ_MOTION_THREADS - 1);   // loops that vote run whole waves
    uint32_t* const cbits = wz_motion_lds;
    uint16_t* const labels = reinterpret_cast<uint16_t*>(wz_motion_lds + cwords);
    uint32_t* const count2 = wz_motion_lds + cwords + lwords;   // two counts a word
    const uint16_t* const count = reinterpret_cast<const uint16_t*>(count2);
    uint32_t* const keys = c.scratch;   // [cells]: there are no more components than cells
    const uint16_t* __restrict__ const now = c.now;
    const uint16_t* __restrict__ const ref = c.ref;

    // 1. C: a wave holds 64 consecutive cells, its vote is two words of the bit map (four steps' loads are in flight together)
    if (tid < WZ_MOTION_CANDIDATES) cand_key[tid] = 0u;
    if (tid == 0) n_keys = 0u, row_lo = INT_MAX, row_hi = -1;
    if (AGE && tid == 0) n_active = n_held = 0u;
    if (MASK && tid == 0) n_ignored = 0u;
    for (int i = tid; i < lwords; i += WZ_MOTION_THREADS) count2[i] = 0u;
    __syncthreads();
    // (AGE) with a hold the age byte is the third load of a step, the vote is "changed or age > 0", and every cell's decayed age is written
    // here, before any early exit: max(hold where the cell changed, age - 1 where there was one)
    const uint8_t* __restrict__ const age_in = c.age_in;
    const bool has_ref = !AGE || ref != nullptr, has_age = aged && age_in != nullptr;
    int active = 0, held = 0;   // lane 0 of a wave: its votes' popcounts
    // (MASK) the wave's 64 cells of a step begin at a multiple of 64: their mask bits are word (i - lane) >> 6, bit `lane` this lane's
    const unsigned long long* __restrict__ const ign = MASK ? c.ignore : nullptr;
    int ignored = 0;
    for (int base = 0; base < span; base += 4 * WZ_MOTION_THREADS) {
        int a[4], b[4], g[4];
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * WZ_MOTION_THREADS + tid;
            a[u] = i < cells ? (int)now[i] : 0;
            b[u] = i < cells && has_ref ? (int)ref[i] : 0;
            g[u] = AGE && has_age && i < cells ? (int)age_in[i] : 0;
            m[u] = MASK && ign && i - lane < cells ? ign[(i - lane) >> 6] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = base + u * WZ_MOTION_THREADS + tid;
            const int y = i / gw, x = i - y * gw;
            const int npix = min(WZ_GATE_CELL, c.W - WZ_GATE_CELL * x) * min(WZ_GATE_CELL, c.H - WZ_GATE_CELL * y);
            const int d = a[u] - b[u];
            const bool differs = i < cells && has_ref && (d < 0 ? -d : d) > c.thr * npix;
            const bool masked = MASK && ((m[u] >> lane) & 1ull) != 0ull;
            const bool changed = differs && !masked;
            if (MASK) ignored += __popcll(__ballot(differs && masked));
            const unsigned long long vote = __ballot(changed || (AGE && g[u] > 0));
            if (AGE && aged) {
                if (i < cells) c.age_out[i] = (uint8_t)max(changed ? c.hold : 0, g[u] > 0 ? g[u] - 1 : 0);
                const unsigned long long moved = __ballot(changed);
                active += __popcll(vote);
                held += __popcll(vote & ~moved);
            }
            const int w0 = (i - lane) >> 5;
            if (lane == 0 && w0 < cwords) {
                cbits[w0] = (uint32_t)vote;
                cbits[w0 + 1] = (uint32_t)(vote >> 32);
                if (vote) {
                    atomicMin(&row_lo, (i - lane + __ffsll((long long)vote) - 1) / gw);
                    atomicMax(&row_hi, (i - lane + 63 - __clzll((long long)vote)) / gw);
                }
            }
        }
    }
    if (AGE && aged && lane == 0) {
        atomicAdd(&n_active, (uint32_t)active);
        atomicAdd(&n_held, (uint32_t)held);
    }
    if (MASK && lane == 0 && ignored) atomicAdd(&n_ignored, (uint32_t)ignored);
    __syncthreads();
    if (row_hi < 0) {   // a still picture (read behind the barrier: the same for every thread); (MASK) also: every changed cell was ignored
        if (tid < RESULT_WORDS) out_words[tid] = MASK && tid == IGNORED_WORD ? n_ignored : 0u;
        return;
    }
    // Every step below looks at rows y_lo .. y_hi only: the rows D can reach and one more on either side, whose labels the scan reads.
    const int dil = c.dilate;
    const int y_lo = max(0, row_lo - dil - 1), y_hi = min(c.gh - 1, row_hi + dil + 1);
    const int lo = y_lo * gw, hi = (y_hi + 1) * gw;
    const int lo64 = lo & ~63, hi64 = lo64 + ((hi - lo64 + WZ_MOTION_THREADS - 1) & ~(WZ_MOTION_THREADS - 1));   // ... in whole waves, for the loops that vote

    // 2. D, and every D cell its own root
    for (WzMotionWalk w(lo + tid, gw); w.i < hi; w.next()) {
        const int i = w.i, x = w.x, y = w.y;
        // 25 reads that do not wait for each other: an offset beyond `dil` or the grid is clamped onto a cell of the neighbourhood
        const int x_lo = max(0, x - dil), x_hi = min(gw - 1, x + dil), yy_lo = max(0, y - dil), yy_hi = min(c.gh - 1, y + dil);
        uint32_t on = 0u;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int j = min(max(y + dy, yy_lo), yy_hi) * gw + min(max(x + dx, x_lo), x_hi);
                on |= cbits[j >> 5] >> (j & 31);
            }
        labels[i] = (on & 1u) ? (uint16_t)i : (uint16_t)WZ_MOTION_BG;
    }
    __syncthreads();

    // 3. the components (see the head of this file)
    int rounds = 0;
    for (;; ++rounds) {
        if (tid == 0) again = 0;
        __syncthreads();
        for (WzMotionWalk w(lo + tid, gw); w.i < hi; w.next()) {
            const int i = w.i, x = w.x, y = w.y;
            const uint32_t l = labels[i];
            if (l == WZ_MOTION_BG) continue;
            uint32_t m = l;   // (WZ_MOTION_BG is above every label; a neighbour beyond the grid is clamped onto a cell of the neighbourhood)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx)
                    m = min(m, (uint32_t)labels[min(max(y + dy, 0), c.gh - 1) * gw + min(max(x + dx, 0), gw - 1)]);
            if (m < l) {
                wz_motion_min16(labels, l, m);
                again = 1;
            }
        }
        __syncthreads();
        const int more = again;   // (read by every thread before the barrier below; thread 0 clears it behind that barrier)
        for (int i = lo + tid; i < hi; i += WZ_MOTION_THREADS) {
            const uint32_t l = labels[i];
            if (l == WZ_MOTION_BG) continue;
            uint32_t r = l;
            for (uint32_t p = labels[r]; p != r; p = labels[r]) r = p;   // label[r] < r until the root: the walk ends
            if (r != l) labels[i] = (uint16_t)r;
        }
        __syncthreads();
        if (!more) break;
    }

    // 4. n of every component, at its root: a wave whose C cells share a root adds once (n <= 32768: two counts share a word, none carries)
    for (int i = lo64 + tid; i < hi64; i += WZ_MOTION_THREADS) {
        const bool cc = i < cells && ((cbits[i >> 5] >> (i & 31)) & 1u);
        const uint32_t r = cc ? labels[i] : 0u;
        const unsigned long long act = __ballot(cc);
        if (!act) continue;
        const int first = __ffsll((long long)act) - 1;
        const uint32_t r0 = __shfl(r, first);
        if (__ballot(cc && r != r0) == 0ull) {
            if (lane == first) atomicAdd(&count2[r0 >> 1], (uint32_t)__popcll(act) << ((r0 & 1u) * 16u));
        } else if (cc) {
            atomicAdd(&count2[r >> 1], 1u << ((r & 1u) * 16u));
        }
    }
    __syncthreads();

    // 5. the keys of the components with n >= min_cells, in any order (keys are unique: the ranking does not depend on it)
    for (int i = lo + tid; i < hi; i += WZ_MOTION_THREADS) {
        if (labels[i] != (uint32_t)i) continue;
        const uint32_t n = count[i];
        if ((int)n < c.min_cells) continue;
        const uint32_t at = atomicAdd(&n_keys, 1u), key = (n << 15) | (uint32_t)(32767 - i);
        if (at < WZ_MOTION_NEAR_KEYS) near_keys[at] = key;
        keys[at] = key;
    }
    __threadfence();   // (the keys in device memory are at the L2 before any other thread asks for them)
    __syncthreads();

    // 6. ranking.  Up to WZ_MOTION_NEAR_KEYS components: a key's rank is the number of keys above it, counted in LDS.  More (a picture of
    // noise): the largest key below the previous one, WZ_MOTION_CANDIDATES times, over the keys in device memory.  The same ranks either way.
    const int n_comp = (int)n_keys;
    const int n_cand = min(WZ_MOTION_CANDIDATES, n_comp);
    if (n_comp <= WZ_MOTION_NEAR_KEYS) {
        for (int k = tid; k < n_comp; k += WZ_MOTION_THREADS) {
            const uint32_t v = near_keys[k];
            int rank = 0;
#pragma unroll 8
            for (int j = 0; j < n_comp; ++j) rank += near_keys[j] > v ? 1 : 0;
            if (rank < WZ_MOTION_CANDIDATES) cand_key[rank] = v;
        }
        __syncthreads();
    } else {
        uint32_t prev = 0xffffffffu;
        for (int r = 0; r < n_cand; ++r) {
            uint32_t mx = 0u;
            for (int k = tid; k < n_comp; k += WZ_MOTION_THREADS) {
                const uint32_t v = wz_motion_load(&keys[k]);
                if (v < prev && v > mx) mx = v;
            }
            for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
            if (lane == 0 && mx) atomicMax(&cand_key[r], mx);
            __syncthreads();
            prev = cand_key[r];
        }
    }

    // 7. the candidates' cell boxes: a ranked root carries its rank where its count was (a count stays below WZ_MOTION_RANKED)
    uint16_t* const mark = reinterpret_cast<uint16_t*>(count2);
    if (tid < n_cand) {
        mark[32767 - (int)(cand_key[tid] & 0x7fffu)] = (uint16_t)(WZ_MOTION_RANKED | (uint32_t)tid);
        box[tid][0] = INT_MAX; box[tid][1] = -1; box[tid][2] = INT_MAX; box[tid][3] = -1;
    }
    __syncthreads();
    for (WzMotionWalk w(lo64 + tid, gw); w.i < hi64; w.next()) {
        const int i = w.i, x = w.x, y = w.y;
        int r = -1;
        if (i >= lo && i < hi) {
            const uint32_t l = labels[i];
            if (l != WZ_MOTION_BG) {
                const uint32_t v = count[l];
                if (v >= WZ_MOTION_RANKED) r = (int)(v & 63u);
            }
        }
        const bool on = r >= 0;
        const unsigned long long act = __ballot(on);
        if (!act) continue;
        const int first = __ffsll((long long)act) - 1;
        const int r0 = __shfl(r, first);
        if (__ballot(on && r != r0) == 0ull) {   // one component in the wave: reduce, then four LDS atomics
            int x0 = on ? x : INT_MAX, x1 = on ? x : -1, y0 = on ? y : INT_MAX, y1 = on ? y : -1;
            for (int off = 32; off > 0; off >>= 1) {
                x0 = min(x0, __shfl_xor(x0, off));
                x1 = max(x1, __shfl_xor(x1, off));
                y0 = min(y0, __shfl_xor(y0, off));
                y1 = max(y1, __shfl_xor(y1, off));
            }
            if (lane == first) {
                atomicMin(&box[r0][0], x0); atomicMax(&box[r0][1], x1);
                atomicMin(&box[r0][2], y0); atomicMax(&box[r0][3], y1);
            }
        } else if (on) {
            atomicMin(&box[r][0], x); atomicMax(&box[r][1], x);
            atomicMin(&box[r][2], y); atomicMax(&box[r][3], y);
        }
    }
    __syncthreads();

    // 8. the walk, one wave: lane r holds candidate r.  The lowest rank still alive is covered by no region accepted so far, so it is
    // accepted; every candidate whose tight rectangle its final rectangle covers dies with it -- what walking them one by one does.
    if (tid < 64) {
        const bool valid = tid < n_cand;
        const int r = valid ? tid : 0;
        const int tx0 = max(0, WZ_GATE_CELL * box[r][0] - c.pad), tx1 = min(c.W, min(c.W, WZ_GATE_CELL * (box[r][1] + 1)) + c.pad);
        const int ty0 = max(0, WZ_GATE_CELL * box[r][2] - c.pad), ty1 = min(c.H, min(c.H, WZ_GATE_CELL * (box[r][3] + 1)) + c.pad);
        int fx0 = tx0, fx1 = tx1, fy0 = ty0, fy1 = ty1;
        wz_motion_axis(fx0, fx1, c.W, c.min_side, c.even_x);
        wz_motion_axis(fy0, fy1, c.H, c.min_side, c.even_y);
        const int32_t n = (int32_t)(cand_key[r] >> 15);
        bool alive = valid;
        int nr = 0;
        for (unsigned long long live = __ballot(alive); live && nr < c.max_regions; live = __ballot(alive), ++nr) {
            const int j = __ffsll((long long)live) - 1;
            const int ax0 = __shfl(fx0, j), ax1 = __shfl(fx1, j), ay0 = __shfl(fy0, j), ay1 = __shfl(fy1, j);
            if (tid == j) {
                result.regions[nr].x0 = fx0; result.regions[nr].y0 = fy0; result.regions[nr].w = fx1 - fx0; result.regions[nr].h = fy1 - fy0;
                result.cells[nr] = n;
                alive = false;
            } else if (alive && ax0 <= tx0 && tx1 <= ax1 && ay0 <= ty0 && ty1 <= ay1) {
                alive = false;
            }
        }
        if (tid == 0) {
            result.n_regions = nr;
            result.components = n_comp;
            result.rounds = rounds + 1;
            result.active = aged ? (int32_t)n_active : 0;
            result.held = aged ? (int32_t)n_held : 0;
            result.ignored = MASK ? (int32_t)n_ignored : 0;
        }
        if (tid >= nr && tid < WZ_MOTION_MAX_REGIONS) {
            result.regions[tid].x0 = result.regions[tid].y0 = result.regions[tid].w = result.regions[tid].h = 0;
            result.cells[tid] = 0;
        }
    }
    __syncthreads();
    if (tid < RESULT_WORDS) out_words[tid] = reinterpret_cast<const uint32_t*>(&result)[tid];
}

void wz_launch_motion_regions(const WzMotionCam* cams, int n, int max_cells, WzMotionOut* out, hipStream_t s, bool with_age, bool with_mask) {
    const size_t lds = (size_t)(((max_cells + 63) >> 6) * 2) * 4 + (((size_t)max_cells + 1) & ~(size_t)1) * 4;   // bits, labels, counts
    const auto kernel = with_mask ? (with_age ? wz_k_motion_regions<true, true> : wz_k_motion_regions<false, true>)
                                  : (with_age ? wz_k_motion_regions<true, false> : wz_k_motion_regions<false, false>);
    if (lds > 48 * 1024)   // (more than 11 k cells: past what a launch gets without asking; a CU of gfx950 has 160 KiB)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)n), dim3(WZ_MOTION_THREADS), lds, s, cams, out);
}

// One workgroup per frame of the call; only a frame without a tile is touched.
__global__ __launch_bounds__(128) void wz_k_motion_still(const WzMergeFrame* __restrict__ frames, wz_detection_t* __restrict__ rows,
                                                         uint8_t* __restrict__ pass) {
    const int f = blockIdx.x, tid = threadIdx.x;
    if (frames[f].n_tiles != 0 || tid >= WZ_MAX_DETECTIONS) return;
    wz_detection_t d;
    d.label = 1;
#pragma unroll
    for (int z = 0; z < WZ_MAX_ZONES; ++z) d.zones[z] = 0;
    d._pad = 0;
    d.confidence = 0.0;
    d.x_min = d.y_min = d.x_max = d.y_max = 0;
    rows[(size_t)f * WZ_MAX_DETECTIONS + tid] = d;
    pass[(size_t)f * WZ_MAX_DETECTIONS + tid] = 0;
}

void wz_launch_motion_still(const WzMergeFrame* frames, int n, wz_detection_t* rows, uint8_t* pass, hipStream_t s) {
    hipLaunchKernelGGL(wz_k_motion_still, dim3((unsigned)n), dim3(128), 0, s, frames, rows, pass);
}

// One workgroup per frame of the call; a frame whose camera has no age grid or whose object_hold is 0 does nothing.  Waves take rows, lanes
// stride over the cells of the row's box, clamped to the frame: x1 <= W - 1 gives a column below gw, y1 <= H - 1 a row below gh.
// Rows overlap, so several lanes, of one wave or of several, may meet at a cell.  Each of them stores ONE BYTE, and every one of them the
// same value, object_hold, over an age that only the region launch -- finished long before -- and such stores have written: whichever
// store lands last, the byte ends as max(age, object_hold), and a neighbouring byte is never touched.  The result does not depend on
// scheduling; no atomics, no scratch.
#define WZ_MOTION_STAMP_THREADS 256
__global__ __launch_bounds__(WZ_MOTION_STAMP_THREADS) void wz_k_motion_stamp(const WzMotionCam* __restrict__ cams, const wz_detection_t* __restrict__ rows,
                                                                      const uint8_t* __restrict__ pass) {
    const int f = blockIdx.x, lane = threadIdx.x & 63;
    uint8_t* const age = cams[f].age_out;
    const int to = cams[f].object_hold;
    if (!age || to <= 0) return;
    const int W = cams[f].W, H = cams[f].H, gw = cams[f].gw;
    for (int r = threadIdx.x >> 6; r < WZ_MAX_DETECTIONS; r += WZ_MOTION_STAMP_THREADS / 64) {
        const size_t at = (size_t)f * WZ_MAX_DETECTIONS + r;
        if (pass[at] != 1) continue;
        const int x0 = max(rows[at].x_min, 0), x1 = min(rows[at].x_max, W - 1);
        const int y0 = max(rows[at].y_min, 0), y1 = min(rows[at].y_max, H - 1);
        if (x0 > x1 || y0 > y1) continue;
        const int cx0 = x0 >> 4, cy0 = y0 >> 4, bw = (x1 >> 4) - cx0 + 1, n = bw * ((y1 >> 4) - cy0 + 1);
        for (int k = lane; k < n; k += 64) {
            const int y = k / bw, i = (cy0 + y) * gw + cx0 + (k - y * bw);
            if ((int)age[i] < to) age[i] = (uint8_t)to;
        }
    }
}
static_assert(WZ_GATE_CELL == 16, "wz_k_motion_stamp turns pixels into cells with >> 4");

void wz_launch_motion_stamp(const WzMotionCam* cams, int n, const wz_detection_t* rows, const uint8_t* pass, hipStream_t s) {
    hipLaunchKernelGGL(wz_k_motion_stamp, dim3((unsigned)n), dim3(WZ_MOTION_STAMP_THREADS), 0, s, cams, rows, pass);
}

// Tiled detection (include/watsor_hip.h: wz_detect_tiled / wz_submit_tiled_device): the two launches around an
// ordinary batch.
//   wz_k_crop_tiles   copies every tile of every frame out of its frame into a contiguous image of the lane's tile staging area -- the
//                     batch behind it sees ordinary frames of size tw x th in the frame's own pixel format.
//   wz_k_merge_tiles  one workgroup per frame: the tiles' Detection rows (written by wz_k_nms, unfiltered, in tile pixel coordinates) are
//                     shifted into frame coordinates, ordered by confidence, thinned by a cross-tile suppression and cut to 100 rows.
// Both are bit-exact stages (tests/tile_oracle.py restates the merge on the CPU): built without fused multiply-add contraction like
// k_post.hip, and the one floating-point operation of the merge is a correctly rounded double division.
#include "wz_common.h"

// ---------------------------------------------------------------------------------------------
// crop: one to three rectangular byte copies per tile (the host expands a tile into planes: wz_engine.hip, tile_planes)
// ---------------------------------------------------------------------------------------------
// A thread owns one 16-byte aligned word of the DESTINATION (the tile image is contiguous: rows * row_bytes bytes).  Where that word lies
// inside one source row it is filled by wide loads -- one 16-byte load when the source address allows it, four dwords when it is 4-byte
// aligned, five aligned dwords and a byte shift when it is not and the five lie inside the row -- and stored at once; the ragged
// ends (the plane's first and last word, words that straddle two rows, misaligned words next to a row's end) go byte by byte.
// No byte outside the source rectangle's rows is read, none outside [dst, dst + rows * row_bytes) written.
__global__ __launch_bounds__(256) void wz_k_crop_tiles(WzCropPack pack) {
    const WzCropPlane pl = pack.p[blockIdx.y];
    const uint32_t total = (uint32_t)pl.rows * (uint32_t)pl.row_bytes;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(pl.dst);
    const uint32_t head = (uint32_t)(d0 & 15u);
    const uint32_t chunks = (head + total + 15u) >> 4;
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= chunks) return;
    const int64_t lo = (int64_t)k * 16 - head, hi = lo + 16;   // this word's bytes, counted from the plane's first
    const uint32_t rb = (uint32_t)pl.row_bytes;
    if (lo >= 0 && hi <= (int64_t)total) {
        const uint32_t row = (uint32_t)lo / rb, col = (uint32_t)lo - row * rb;
        if (col + 16u <= rb) {
            const uint8_t* rs = pl.src + (size_t)row * (size_t)pl.src_pitch;   // the row's first byte
            const uint8_t* s = rs + col;
            const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 3u);
            uint4 v;
            bool wide = true;
            if (m == 0) {
                if ((reinterpret_cast<uintptr_t>(s) & 15u) == 0) {
                    v = *reinterpret_cast<const uint4*>(s);
                } else {
                    const uint32_t* q = reinterpret_cast<const uint32_t*>(s);
                    v = make_uint4(q[0], q[1], q[2], q[3]);
                }
            } else if (s - m >= rs && s - m + 20 <= rs + rb) {
                const uint32_t* q = reinterpret_cast<const uint32_t*>(s - m);
                const uint32_t a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
                const uint32_t sr = 8u * m, sl = 32u - sr;
                v = make_uint4((a >> sr) | (b << sl), (b >> sr) | (c << sl), (c >> sr) | (d << sl), (d >> sr) | (e << sl));
            } else {
                wide = false;
            }
            if (wide) {
                *reinterpret_cast<uint4*>(pl.dst + lo) = v;
                return;
            }
        }
    }
    const uint32_t b0 = lo < 0 ? 0u : (uint32_t)lo, b1 = hi > (int64_t)total ? total : (uint32_t)hi;
    uint32_t row = b0 / rb, col = b0 - row * rb;
    for (uint32_t b = b0; b < b1; ++b) {
        pl.dst[b] = pl.src[(size_t)row * (size_t)pl.src_pitch + col];
        if (++col == rb) col = 0, ++row;
    }
}

void wz_launch_crop_tiles(const WzCropPlane* planes, int n, hipStream_t s) {
    for (int first = 0; first < n; first += WZ_CROP_PACK) {
        const int m = n - first < WZ_CROP_PACK ? n - first : WZ_CROP_PACK;
        WzCropPack pack;
        uint32_t chunks = 1;
        for (int i = 0; i < WZ_CROP_PACK; ++i) {
            pack.p[i] = planes[first + (i < m ? i : 0)];
            const uint32_t c = (uint32_t)pack.p[i].rows * (uint32_t)pack.p[i].row_bytes / 16u + 2u;
            if (c > chunks) chunks = c;
        }
        hipLaunchKernelGGL(wz_k_crop_tiles, dim3((chunks + 255u) / 256u, (unsigned)m), dim3(256), 0, s, pack);
    }
}

// ---------------------------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------------------------
#define WZ_MERGE_THREADS 1024

struct MergeBox {
    int32_t label, x_min, y_min, x_max, y_max;
};
__device__ __forceinline__ long long wz_merge_area(const MergeBox& b) {
    return ((long long)b.x_max - (long long)b.x_min) * ((long long)b.y_max - (long long)b.y_min);
}
// do two rows of the same label show the same object?  int64 arithmetic, one correctly rounded double division per test
__device__ __forceinline__ bool wz_merge_match(const MergeBox& a, long long a1, const MergeBox& b, long long a2, double iou_thr, double ios_thr) {
    long long ix = (long long)min(a.x_max, b.x_max) - (long long)max(a.x_min, b.x_min);
    long long iy = (long long)min(a.y_max, b.y_max) - (long long)max(a.y_min, b.y_min);
    ix = ix > 0 ? ix : 0;
    iy = iy > 0 ? iy : 0;
    const long long inter = ix * iy, uni = a1 + a2 - inter, amin = a1 < a2 ? a1 : a2;
    if (iou_thr < 1.0 && uni > 0 && (double)inter / (double)uni > iou_thr) return true;
    return ios_thr < 1.0 && amin > 0 && (double)inter / (double)amin > ios_thr;
}

// LDS: key[np2] (8 bytes) + idx[np2] (2 bytes) of the frame with the most tiles in the launch; np2 = the frame's 100 * n_tiles rounded up to a
// power of two (at least 128).  A key is the bit pattern of the row's confidence where the row is a candidate (label > 0, confidence > 0: a
// positive double's bits order like its value) and 0 where it is not; idx is the row's number t * 100 + r.
__global__ __launch_bounds__(WZ_MERGE_THREADS) void wz_k_merge_tiles(const WzMergeFrame* __restrict__ frames, const int32_t* __restrict__ origins,
                                                                     const wz_detection_t* tile_rows, WzMergeCand* cands,
                                                                     double iou_thr, double ios_thr, wz_detection_t* __restrict__ rows,
                                                                     uint8_t* __restrict__ pass) {
    extern __shared__ unsigned long long wz_merge_lds[];
    __shared__ MergeBox kept[WZ_MAX_DETECTIONS];
    __shared__ long long kept_area[WZ_MAX_DETECTIONS];
    __shared__ double kept_conf[WZ_MAX_DETECTIONS];
    __shared__ int n_cand, n_kept;

    const int f = blockIdx.x, tid = threadIdx.x;
    const WzMergeFrame fr = frames[f];
    const int nc = fr.n_tiles * WZ_MAX_DETECTIONS;
    int np2 = 128;
    while (np2 < nc) np2 <<= 1;
    unsigned long long* key = wz_merge_lds;
    uint16_t* idx = reinterpret_cast<uint16_t*>(wz_merge_lds + np2);
    const wz_detection_t* src = tile_rows + (size_t)fr.first * WZ_MAX_DETECTIONS;
    WzMergeCand* cand = cands + (size_t)fr.first * WZ_MAX_DETECTIONS;
    if (tid == 0) n_cand = 0, n_kept = 0;
    __syncthreads();

    // 1. every row into frame coordinates (int32, nothing clamped) and its sort key
    for (int c = tid; c < np2; c += WZ_MERGE_THREADS) {
        unsigned long long k = 0;
        if (c < nc) {
            const int t = c / WZ_MAX_DETECTIONS;
            const int32_t ox = origins[2 * (fr.first + t)], oy = origins[2 * (fr.first + t) + 1];
            const wz_detection_t& r = src[c];
            WzMergeCand m;
            m.label = r.label;
            m.confidence = r.confidence;
            m.x_min = (int32_t)((uint32_t)r.x_min + (uint32_t)ox);
            m.y_min = (int32_t)((uint32_t)r.y_min + (uint32_t)oy);
            m.x_max = (int32_t)((uint32_t)r.x_max + (uint32_t)ox);
            m.y_max = (int32_t)((uint32_t)r.y_max + (uint32_t)oy);
            m._pad = 0;
            cand[c] = m;
            if (m.label > 0 && m.confidence > 0.0) {
                k = (unsigned long long)__double_as_longlong(m.confidence);
                atomicAdd(&n_cand, 1);
            }
        }
        key[c] = k;
        idx[c] = c < nc ? (uint16_t)c : (uint16_t)0xffff;
    }
    __syncthreads();

    // 2. bitonic sort: confidence descending, then row number ascending (tile, then row); rows that are no candidates end up last
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += WZ_MERGE_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long ka = key[i], kb = key[l];
                    const uint16_t ia = idx[i], ib = idx[l];
                    const bool a_first = ka > kb || (ka == kb && ia < ib);
                    if (((i & k) == 0) != a_first) {
                        key[i] = kb; key[l] = ka;
                        idx[i] = ib; idx[l] = ia;
                    }
                }
            }
            __syncthreads();
        }

    // 3. the walk, on one wave: 64 candidates at a time, each lane tests its own against the rows kept so far; the survivors are taken in
    // order, each one kept and tested against the later survivors of its batch
    if (tid < 64) {
        const int total = n_cand;
        int nk = 0;
        WzMergeCand nxt;
        nxt.label = 0; nxt.x_min = nxt.y_min = nxt.x_max = nxt.y_max = 0; nxt._pad = 0; nxt.confidence = 0.0;
        if (tid < total) nxt = cand[idx[tid]];
        for (int base = 0; base < total && nk < WZ_MAX_DETECTIONS; base += 64) {
            const WzMergeCand cur = nxt;
            if (base + 64 + tid < total) nxt = cand[idx[base + 64 + tid]];   // (in flight while this batch is walked)
            const MergeBox mine = {cur.label, cur.x_min, cur.y_min, cur.x_max, cur.y_max};
            const long long area = wz_merge_area(mine);
            bool alive = base + tid < total;
            for (int q = 0; q < nk; ++q)
                if (alive && kept[q].label == mine.label && wz_merge_match(kept[q], kept_area[q], mine, area, iou_thr, ios_thr)) alive = false;
            unsigned long long live = __ballot(alive);
            while (live && nk < WZ_MAX_DETECTIONS) {
                const int j = __ffsll((long long)live) - 1;
                MergeBox kb;
                kb.label = __shfl(mine.label, j);
                kb.x_min = __shfl(mine.x_min, j);
                kb.y_min = __shfl(mine.y_min, j);
                kb.x_max = __shfl(mine.x_max, j);
                kb.y_max = __shfl(mine.y_max, j);
                const long long ka = wz_merge_area(kb);
                if (tid == j) {
                    kept[nk] = mine;
                    kept_area[nk] = area;
                    kept_conf[nk] = cur.confidence;
                    alive = false;
                } else if (alive && tid > j && kb.label == mine.label && wz_merge_match(kb, ka, mine, area, iou_thr, ios_thr)) {
                    alive = false;
                }
                ++nk;
                live = __ballot(alive);
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (tid == 0) n_kept = nk;
    }
    __syncthreads();

    // 4. the kept rows in order, zones 0; the engine's padding row behind them.  The camera filter runs behind this kernel
    // (wz_k_filter_rows, in place); until then pass = (label > 0), which is what stays for a frame without one.
    if (tid < WZ_MAX_DETECTIONS) {
        wz_detection_t d;
        d.label = 1;
#pragma unroll
        for (int z = 0; z < WZ_MAX_ZONES; ++z) d.zones[z] = 0;
        d._pad = 0;
        d.confidence = 0.0;
        d.x_min = d.y_min = d.x_max = d.y_max = 0;
        if (tid < n_kept) {
            d.label = kept[tid].label;
            d.confidence = kept_conf[tid];
            d.x_min = kept[tid].x_min; d.y_min = kept[tid].y_min; d.x_max = kept[tid].x_max; d.y_max = kept[tid].y_max;
        }
        rows[(size_t)f * WZ_MAX_DETECTIONS + tid] = d;
        pass[(size_t)f * WZ_MAX_DETECTIONS + tid] = d.label > 0 ? 1 : 0;
    }
}

void wz_launch_merge_tiles(const WzMergeFrame* frames, const int32_t* origins, const wz_detection_t* tile_rows, WzMergeCand* cands, int n,
                           int max_tiles, double iou_thr, double ios_thr, wz_detection_t* rows, uint8_t* pass, hipStream_t s) {
    int np2 = 128;
    while (np2 < max_tiles * WZ_MAX_DETECTIONS) np2 <<= 1;
    const size_t lds = (size_t)np2 * 10;
    if (lds > 48 * 1024)   // (more than 40 tiles in one frame: past what a launch gets without asking)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wz_k_merge_tiles), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(wz_k_merge_tiles, dim3(n), dim3(WZ_MERGE_THREADS), lds, s, frames, origins, tile_rows, cands, iou_thr, ios_thr, rows, pass);
}

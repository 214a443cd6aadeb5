// Tiled, gated, motion-region and tiled frame-table detection (include/watsor_hip.h; DESIGN.md sections 15 - 17b and 19): eager launches of
// k_tiles.hip, k_gate.hip and k_motion.hip around run_batch.  wz_engine.hip knows nothing of this file but TileLane / GateLane / MotionLane /
// GateCam's and MotionCam's release, the lane's `tile.tiled` and merged rows (`tile.trows`, `tile.tpass`) and submit_bound_tiles (wz_engine.h).
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <numeric>

#include "wz_engine.h"

typedef wz_engine::GateCam GateCam;
typedef wz_engine::MotionCam MotionCam;

static int cells_of(int px) { return (px + WZ_GATE_CELL - 1) / WZ_GATE_CELL; }
static size_t gate_cells_of(int w, int h) { return (size_t)cells_of(w) * (size_t)cells_of(h); }
// Ignore masks: wz_ignore_cells' bytes as the kernels read them, cell i at bit (i & 63) of 64-bit word (i >> 6) --
// which, little-endian, is bit (i & 31) of 32-bit word (i >> 5): wz_k_motion_regions reads the former, wz_k_tile_activity the latter
static size_t ignore_words_of(size_t cells) { return (cells + 63) >> 6; }
static void pack_cell_bits(const uint8_t* cells, size_t n, unsigned long long* words) {
    std::fill(words, words + ignore_words_of(n), 0ull);
    for (size_t i = 0; i < n; ++i)
        if (cells[i]) words[i >> 6] |= 1ull << (i & 63);
}

// ---- lane state
// Everything a lane needs for one kind of call, allocated the first time it sees one (an engine that never does uses no byte of it): built
// aside and moved in, so that a failure leaves the lane without any of it (wz_engine.h: DevBlock, MappedBlock, MetaBlock).
int TileLane::alloc(wz_engine* e) {
    if (d_tiles) return WZ_OK;
    const size_t nb = (size_t)e->max_batch, rows = nb * WZ_MAX_DETECTIONS;
    TileLane t;
    hipError_t err = t.d_tiles.alloc(e->frame_stride * nb);
    if (err == hipSuccess) err = t.d_tcand.alloc(rows);
    if (err == hipSuccess) err = t.trows.alloc(rows);
    if (err == hipSuccess) err = t.tpass.alloc(rows);
    if (err == hipSuccess) err = t.meta.alloc(nb);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "tile staging of a lane (%zu bytes): %s", e->frame_stride * nb, hipGetErrorString(err));
    t.tiled = tiled;
    *this = std::move(t);
    return WZ_OK;
}

int GateLane::alloc(wz_engine* e) {
    if (d_gnow) return WZ_OK;
    const size_t nb = (size_t)e->max_batch;
    GateLane g;
    hipError_t err = g.d_gnow.alloc(gate_cells_of(e->max_w, e->max_h) * nb);
    if (err == hipSuccess) err = g.d_grows.alloc(WZ_MAX_DETECTIONS * nb);
    if (err == hipSuccess) err = g.d_gcount.alloc(2 * nb);
    if (err == hipSuccess) err = lane0_fill(e, g.d_gcount, 0, 8 * nb);
    if (err == hipSuccess) err = g.meta.alloc(nb);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "gate scratch of a lane: %s", hipGetErrorString(err));
    *this = std::move(g);
    return WZ_OK;
}

int MotionLane::alloc(wz_engine* e) {
    if (d_mscratch) return WZ_OK;
    const size_t nb = (size_t)e->max_batch;
    MotionLane m;
    m.cam_words = std::min((size_t)WZ_MOTION_MAX_CELLS, gate_cells_of(e->max_w, e->max_h));
    hipError_t err = m.d_mscratch.alloc(m.cam_words * nb);
    if (err == hipSuccess) err = m.d_mcount.alloc(2 * nb);
    if (err == hipSuccess) err = lane0_fill(e, m.d_mcount, 0, 8 * nb);
    if (err == hipSuccess) err = m.meta.alloc(nb);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "motion scratch of a lane: %s", hipGetErrorString(err));
    *this = std::move(m);
    return WZ_OK;
}

// ---- rectangles
// Why rectangle t of a w x h frame of format word fmt cannot be cut, or nullptr
static const char* tile_refusal(const wz_tile_t& t, int w, int h, int fmt) {
    if (t.w < 1 || t.h < 1 || t.x0 < 0 || t.y0 < 0) return "origin and size must not be negative, the size not zero";
    if ((int64_t)t.x0 + t.w > w || (int64_t)t.y0 + t.h > h) return "the rectangle leaves the frame";
    const int base = fmt & WZ_FMT_BASE_MASK;
    const bool ten = base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10;
    if ((ten || base == WZ_FMT_NV12 || base == WZ_FMT_I420) && ((t.x0 | t.y0 | t.w | t.h) & 1))
        return ten ? "P010 / YUV420P10 need even x0, y0, w and h" : "NV12 / I420 need even x0, y0, w and h";
    if ((base == WZ_FMT_YUYV422 || base == WZ_FMT_UYVY422) && ((t.x0 | t.w) & 1)) return "YUYV422 / UYVY422 need even x0 and w";
    if (!wz_frame_bytes(t.w, t.h, fmt)) return fmt_refusal(t.w, t.h, fmt);
    return nullptr;
}
// ... and whether the engine takes it: tile_refusal plus the engine's size limit, for rectangle `idx` of `what` number `id` ("frame" |
// "camera" | "frame-table entry"), which is w x h in format word fmt.  WZ_OK, or the code with wz_last_error set.
static int tile_fits(const wz_engine* e, const char* what, int id, int w, int h, int fmt, int idx, const wz_tile_t& r) {
    const char* why = tile_refusal(r, w, h, fmt);
    if (why) return wz_set_error(WZ_EINVAL, "%s %d (%dx%d, format 0x%x), tile %d (%d, %d, %d x %d): %s", what, id, w, h, fmt, idx, r.x0, r.y0, r.w, r.h, why);
    if (r.w > e->max_w || r.h > e->max_h || (size_t)r.w * r.h * 3 > e->frame_stride)
        return wz_set_error(WZ_ELIMIT, "%s %d, tile %d is %dx%d, engine was created for at most %dx%d", what, id, idx, r.w, r.h, e->max_w, e->max_h);
    return WZ_OK;
}

// The one to three rectangular byte copies that cut rectangle t out of a w x h frame at `src` into a contiguous image at `dst`.
static void tile_planes(const uint8_t* src, int w, int h, int fmt, const wz_tile_t& t, uint8_t* dst, std::vector<WzCropPlane>& out) {
    const int base = fmt & WZ_FMT_BASE_MASK;
    const size_t W = (size_t)w, H = (size_t)h;
    const bool ten = base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10;   // NV12's / I420's planes with two bytes a sample
    if (ten || base == WZ_FMT_NV12 || base == WZ_FMT_I420) {
        const int s = ten ? 2 : 1;
        out.push_back({src + ((size_t)t.y0 * W + t.x0) * s, dst, w * s, t.w * s, t.h, 0});
        const uint8_t* chroma = src + W * H * s;
        uint8_t* dc = dst + (size_t)t.w * t.h * s;
        if (base == WZ_FMT_NV12 || base == WZ_FMT_P010) {   // the (U, V) pair of chroma column x0 / 2 lies x0 samples into its row of w
            out.push_back({chroma + ((size_t)(t.y0 / 2) * W + t.x0) * s, dc, w * s, t.w * s, t.h / 2, 0});
        } else {
            const size_t cw = W / 2, ch = H / 2, off = ((size_t)(t.y0 / 2) * cw + t.x0 / 2) * s;
            out.push_back({chroma + off, dc, w / 2 * s, t.w / 2 * s, t.h / 2, 0});
            out.push_back({chroma + cw * ch * s + off, dc + (size_t)(t.w / 2) * (t.h / 2) * s, w / 2 * s, t.w / 2 * s, t.h / 2, 0});
        }
        return;
    }
    const int bpp = (base == WZ_FMT_RGB24 || base == WZ_FMT_BGR24) ? 3 : (base == WZ_FMT_GRAY8 ? 1 : 2);
    out.push_back({src + ((size_t)t.y0 * W + t.x0) * bpp, dst, w * bpp, t.w * bpp, t.h, 0});
}

// What the activity kernel reads of rectangle t of a frame w pixels wide at `src`: the luma-bearing bytes of its rows
static void gate_tile(const uint8_t* src, int w, int fmt, const wz_tile_t& t, WzGateTile& g) {
    const int base = fmt & WZ_FMT_BASE_MASK;
    const bool rgb = base == WZ_FMT_RGB24 || base == WZ_FMT_BGR24, yuy = base == WZ_FMT_YUYV422 || base == WZ_FMT_UYVY422;
    const bool ten = base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10;   // (the luma plane is the frame's first w x h words)
    const int bpp = rgb ? 3 : (yuy || ten) ? 2 : 1;   // (NV12 / I420: the luma plane is the frame's first w x h bytes)
    g.src = src + ((size_t)t.y0 * (size_t)w + t.x0) * bpp;
    g.pitch = w * bpp;
    g.row_bytes = t.w * bpp;
    g.tw = t.w;
    g.th = t.h;
    g.cols = cells_of(t.w);
    g.crows = cells_of(t.h);
    // The 10-bit formats are gated on the top 8 bits of a sample, so that sums and threshold keep their 8-bit meaning: of a P010 word
    // (sample << 6) that is its second byte -- UYVY's odd bytes --, of a YUV420P10 word bits 2 .. 9 (WZ_GATE_LOW10).
    g.mode = base == WZ_FMT_RGB24 ? WZ_GATE_RGB : base == WZ_FMT_BGR24 ? WZ_GATE_BGR : base == WZ_FMT_YUYV422 ? WZ_GATE_YUYV
             : (base == WZ_FMT_UYVY422 || base == WZ_FMT_P010) ? WZ_GATE_UYVY : base == WZ_FMT_YUV420P10 ? WZ_GATE_LOW10 : WZ_GATE_GRAY;
    g.ignore = nullptr;   // (no mask; a gated camera with one adds its tile's bits)
}

// ---- a call, its checks, its plan
// A tiled or gated call.  fmt and (tiled) cam may be null; a tiled call brings n_tiles / tiles, a gated one gets them from its cameras'
// layouts when it is enqueued, a motion one from the region launch; `total`, all its tiles, is what its check leaves (a motion call's: the most
// it can have).
struct TileCall {
    int n;
    const uint8_t* const* frames;
    const int *w, *h, *fmt, *cam;
    const int* n_tiles;
    const wz_tile_t* const* tiles;
    double iou, ios;
    int total;
    int pf(int i) const { return fmt ? fmt[i] : WZ_FMT_RGB24; }
};

static int call_refusal(const wz_engine* e, const char* who, int slot, const TileCall& c, bool tiled) {
    if (!e || !c.frames || !c.w || !c.h || (tiled && (!c.n_tiles || !c.tiles))) return wz_set_error(WZ_EINVAL, "%s: null argument", who);
    return batch_refusal(e, slot, c.n);
}
static int thresholds_refusal(const char* who, const TileCall& c) {
    if (!(c.iou >= 0.0) || !(c.ios >= 0.0)) return wz_set_error(WZ_EINVAL, "%s: the merge thresholds must be numbers >= 0", who);
    return WZ_OK;
}

// Every refusal of a tiled call (include/watsor_hip.h), before anything is enqueued or written.  host: the frames are host frames that
// go through the lane's staging area, which holds max_width x max_height.
static int tiled_check(wz_engine* e, const char* who, int slot, TileCall& c, bool host) {
    WZCHK(call_refusal(e, who, slot, c, true));
    int64_t sum = 0;
    for (int i = 0; i < c.n; ++i) {
        if (c.n_tiles[i] < 1 || c.n_tiles[i] > WZ_MAX_TILES)
            return wz_set_error(WZ_ELIMIT, "frame %d: %d tiles, a frame takes 1 to %d", i, c.n_tiles[i], WZ_MAX_TILES);
        sum += c.n_tiles[i];
    }
    if (sum > e->max_batch) return wz_set_error(WZ_ELIMIT, "%lld tiles in one call exceed max_batch %d", (long long)sum, e->max_batch);
    for (int i = 0; i < c.n; ++i) {
        WZCHK(frame_refusal(e, "frame", i, c.tiles[i] ? c.frames[i] : nullptr, c.w[i], c.h[i], c.pf(i), c.cam ? c.cam[i] : -1,
                            FC_PTR | FC_FMT | (host ? FC_LIMIT : 0) | FC_CAM_ID | FC_CAM_FILTER));
        for (int t = 0; t < c.n_tiles[i]; ++t) WZCHK(tile_fits(e, "frame", i, c.w[i], c.h[i], c.pf(i), t, c.tiles[i][t]));
    }
    c.total = (int)sum;
    return thresholds_refusal(who, c);
}

// What the two kinds of per-camera call -- gated, motion -- bring to their check: the words of its texts, and (by the type of its cameras)
// what a frame of a camera costs in tiles
struct CamKind { const char *name, *what, *setter, *made, *sum; };
static const CamKind GATED = {"gated", "tiles", "wz_set_camera_tiles", "set", ""};
static const CamKind MOTION = {"motion", "motion settings", "wz_set_camera_motion", "made", " (whole_frame + max_regions)"};
static int64_t tiles_of(const GateCam& g) { return (int64_t)g.tiles.size(); }
static int64_t tiles_of(const MotionCam& m) { return m.p.whole_frame + m.p.max_regions; }

// Every refusal of a gated or motion call (include/watsor_hip.h), before anything is enqueued, written, decided or found.  known: the
// engine's cameras of that kind (e may still be null here)
template <class Cam>
static int camera_check(wz_engine* e, std::map<int, Cam> wz_engine::*known, const CamKind& kind, const char* who, int slot, TileCall& c, bool host) {
    int rc = call_refusal(e, who, slot, c, false);
    if (rc != WZ_OK) return rc;
    const int* cam = c.cam;
    if (!cam) return wz_set_error(WZ_EINVAL, "%s: a %s call needs the frames' camera ids", who, kind.name);
    int64_t sum = 0;
    for (int i = 0; i < c.n; ++i) {
        const int w = c.w[i], h = c.h[i], pf = c.pf(i);
        auto refused = [&](unsigned checks) { return (rc = frame_refusal(e, "frame", i, c.frames[i], w, h, pf, cam[i], checks)) != WZ_OK; };
        if (refused(FC_PTR)) return rc;
        const auto it = (e->*known).find(cam[i]);
        if (it == (e->*known).end()) return wz_set_error(WZ_EINVAL, "frame %d: camera %d has no %s (%s first)", i, cam[i], kind.what, kind.setter);
        for (int j = 0; j < i; ++j)
            if (cam[j] == cam[i])
                return wz_set_error(WZ_EINVAL, "frames %d and %d are both camera %d's: one frame of a camera per %s call", j, i, cam[i], kind.name);
        const Cam& s = it->second;
        if (refused(FC_FMT)) return rc;
        if (w != s.w || h != s.h || (pf & WZ_FMT_BASE_MASK) != s.base)
            return wz_set_error(WZ_EINVAL, "frame %d is %dx%d in base format %d but camera %d's %s were %s for %dx%d in base format %d", i, w, h,
                                pf & WZ_FMT_BASE_MASK, cam[i], kind.what, kind.made, s.w, s.h, s.base);
        if (refused((host ? FC_LIMIT : 0) | FC_CAM_FILTER)) return rc;
        sum += tiles_of(s);
    }
    if (sum > e->max_batch)
        return wz_set_error(WZ_ELIMIT, "the %lld tiles configured for the cameras of one call%s exceed max_batch %d", (long long)sum, kind.sum, e->max_batch);
    c.total = (int)sum;
    return thresholds_refusal(who, c);
}

// What a checked call launches: the crop launch's planes and the tiles that run as the batch's frames (in the lane's tile staging area,
// the k-th of them at k * frame_stride), and -- written into the lane's pinned block -- the merge launch's frames and origins.
struct TilePlan {
    std::vector<WzCropPlane> planes;
    std::vector<const uint8_t*> tptr;
    std::vector<int> tw, th, tf;
    std::vector<int> fresh;   // per tile of the call: its index in the batch, -1 where it does not run
    int most = 0;             // the most tiles any frame has
};
// runs: one byte per tile of the call, 0 = the tile does not run (gated calls); null: every tile runs
static void tile_plan(wz_engine* e, Lane& L, const TileCall& c, const uint8_t* runs, TilePlan& y) {
    const TileMeta& meta = L.tile.meta.h;
    y.fresh.assign(c.total, -1);
    y.tptr.reserve(c.total); y.tw.reserve(c.total); y.th.reserve(c.total); y.tf.reserve(c.total);
    int k = 0;
    for (int i = 0; i < c.n; ++i) {
        const int pf = c.pf(i), cam = c.cam ? c.cam[i] : -1;
        meta.frames[i] = {k, c.n_tiles[i], cam < 0 ? -1 : cam, 0};
        y.most = std::max(y.most, c.n_tiles[i]);
        for (int t = 0; t < c.n_tiles[i]; ++t, ++k) {
            const wz_tile_t& r = c.tiles[i][t];
            if (!runs || runs[k]) {
                y.fresh[k] = (int)y.tptr.size();
                uint8_t* dst = L.tile.d_tiles + e->frame_stride * y.tptr.size();
                tile_planes(c.frames[i], c.w[i], c.h[i], pf, r, dst, y.planes);
                y.tptr.push_back(dst); y.tw.push_back(r.w); y.th.push_back(r.h); y.tf.push_back(pf);   // (the colour flags of the frame's format word are its tiles')
            }
            meta.origins[2 * k] = r.x0;
            meta.origins[2 * k + 1] = r.y0;
        }
    }
}

// The plan's tiles as an ordinary batch without cameras: crop, then 100 unfiltered rows per tile, in tile pixel coordinates, in L.hrows.h.
// No tile runs (a gated call of still tiles, a motion call of still frames): no crop, no batch, no status word is this call's.
static int run_tiles(wz_engine* e, int slot, const TilePlan& y) {
    Lane& L = e->lanes[slot];
    if (y.tptr.empty()) {
        L.bound_idx.clear();
        L.n = 0;
        return WZ_OK;
    }
    wz_launch_crop_tiles(y.planes.data(), (int)y.planes.size(), L.stream);
    WZCHK(fill_desc(e, slot, (int)y.tptr.size(), y.tptr.data(), y.tw.data(), y.th.data(), y.tf.data(), nullptr));
    L.rows = e->pre_rows && rows_fit(e, (int)y.tptr.size(), y.tw.data(), y.tf.data());
    return run_batch(e, slot, (int)y.tptr.size());
}

// ... and behind it: the merge of `src` (every tile's rows, in tile order), each frame's camera filter on its merged rows exactly as
// wz_filter_rows applies it, and the lane's event (run_batch recorded it behind the batch: wz_wait / wz_collect must see the merge)
// still: a motion call with a frame that has no tile -- no filter runs on it, it gets the padding rows and pass bytes 0 (k_motion.hip)
// stamp: a motion call with a camera that holds under detections -- the region launch's cameras; last, the cells under the rows that
// passed all of the above are raised in those cameras' age grids
static int merge_tail(wz_engine* e, Lane& L, const TileCall& c, int most, const wz_detection_t* src, bool still = false, const WzMotionCam* stamp = nullptr) {
    TileLane& T = L.tile;
    wz_launch_merge_tiles(T.meta.m.frames, T.meta.m.origins, src, T.d_tcand, c.n, most, c.iou, c.ios, T.trows.d, T.tpass.d, L.stream);
    for (int i = 0; i < c.n; ++i)
        if (c.cam && c.cam[i] >= 0 && e->h_cams[c.cam[i]].enabled && !(still && c.n_tiles[i] == 0))
            wz_launch_filter_rows(e->d_cams, c.cam[i], T.trows.d + (size_t)i * WZ_MAX_DETECTIONS, T.tpass.d + (size_t)i * WZ_MAX_DETECTIONS, L.stream);
    if (still) wz_launch_motion_still(T.meta.m.frames, c.n, T.trows.d, T.tpass.d, L.stream);
    if (stamp) wz_launch_motion_stamp(stamp, c.n, T.trows.d, T.tpass.d, L.stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(L.done, L.stream));
    T.tiled = c.n;
    return WZ_OK;
}

// What gated_enqueue and motion_enqueue derive from their checked call: its cameras' state, in frame order ...
template <class Cam>
static std::vector<Cam*> cams_of(std::map<int, Cam>& known, const TileCall& c) {
    std::vector<Cam*> cams(c.n);
    for (int i = 0; i < c.n; ++i) cams[i] = &known.find(c.cam[i])->second;
    return cams;
}
// ... and, once the frames' rectangles are known, the tiled call on them
static TileCall with_tiles(const TileCall& call, const std::vector<int>& nt, const std::vector<const wz_tile_t*>& tp) {
    TileCall c = call;
    c.n_tiles = nt.data();
    c.tiles = tp.data();
    c.total = std::accumulate(nt.begin(), nt.end(), 0);
    return c;
}

// ---- tiled detection: crop launch -> an ordinary batch over the tiles -> merge launch (k_tiles.hip)
// A checked tiled call on a drained lane, frames in device memory
static int tiled_enqueue(wz_engine* e, int slot, const TileCall& c) {
    Lane& L = e->lanes[slot];
    WZCHK(L.tile.alloc(e));
    TilePlan y;
    tile_plan(e, L, c, nullptr, y);
    WZCHK(run_tiles(e, slot, y));
    return merge_tail(e, L, c, y.most, L.hrows.d);
}

// ---- gated tiled detection: activity launch -> the host decides which tiles run -> crop + batch of those -> commit + merge (k_gate.hip,
// DESIGN.md section 16)
// The host's rule: does tile t of camera g run, given its activity?
static bool gate_runs(const GateCam& g, int t, int activity) {
    return !g.has_ref[t] || activity >= g.gate.min_cells || (g.gate.max_age > 0 && g.skipped[t] >= g.gate.max_age);
}

// A checked gated call on a drained lane, frames in device memory.  Returns once the decision is made; crop, batch, commit, merge and
// filters are enqueued behind it and the lane's event behind them.
static int gated_enqueue(wz_engine* e, int slot, const TileCall& call) {
    Lane& L = e->lanes[slot];
    GateLane& G = L.gate;
    WZCHK(L.tile.alloc(e));
    WZCHK(G.alloc(e));
    const int n = call.n, total = call.total;
    const std::vector<GateCam*> cams = cams_of(e->gate_cams, call);
    std::vector<int> nt(n);
    std::vector<const wz_tile_t*> tp(n);
    for (int i = 0; i < n; ++i) {
        nt[i] = (int)cams[i]->tiles.size();
        tp[i] = cams[i]->tiles.data();
        // another lane's commit launch may still be writing this camera's references and cached rows
        if (cams[i]->lane >= 0 && cams[i]->lane != slot) HIPCHK(hipEventSynchronize(e->lanes[cams[i]->lane].done));
    }
    const TileCall c = with_tiles(call, nt, tp);   // ... with the cameras' rectangles
    // 1. activity of every tile, one launch
    const size_t lane_cells = gate_cells_of(e->max_w, e->max_h);
    WzGateCommit* commits = G.meta.h.commits;
    int32_t* act = G.meta.h.activity;
    int k = 0, crows = 0, cols = 0;
    bool masked = false;   // some camera of the call has an ignore mask
    for (int i = 0; i < n; ++i) {
        GateCam& g = *cams[i];
        masked = masked || g.d_ignore;
        for (int t = 0; t < nt[i]; ++t, ++k) {
            WzGateTile& d = G.meta.h.tiles[k];
            gate_tile(c.frames[i], c.w[i], c.pf(i), g.tiles[t], d);
            if (g.d_ignore) d.ignore = g.d_ignore + g.ignore_off[t];
            d.ref = g.has_ref[t] ? g.d_ref + g.grid_off[t] : nullptr;
            d.now = G.d_gnow + lane_cells * k;
            d.thr = g.gate.pixel_thr;
            crows = std::max(crows, d.crows);
            cols = std::max(cols, d.cols);
            act[k] = 0;
            commits[k] = {g.d_ref + g.grid_off[t], d.now, g.d_rows + (size_t)t * WZ_MAX_DETECTIONS, d.cols * d.crows, -1};   // (fresh: step 2)
        }
    }
    wz_launch_tile_activity(G.meta.m.tiles, total, crows, cols, G.d_gcount, G.meta.m.activity, L.stream, masked);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(L.stream));   // the batch size is a host-side quantity: the decision waits for the counts
    // 2. the decision; the cameras' state changes only once everything is enqueued
    std::vector<uint8_t> runs(total);
    k = 0;
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < nt[i]; ++t, ++k) runs[k] = gate_runs(*cams[i], t, act[k]) ? 1 : 0;
    TilePlan y;
    tile_plan(e, L, c, runs.data(), y);
    for (k = 0; k < total; ++k) commits[k].fresh = y.fresh[k];
    // 3. the tiles that run, as an ordinary batch without cameras (none: no crop, no batch)
    WZCHK(run_tiles(e, slot, y));
    // 4. commit, merge, filters
    wz_launch_gate_commit(G.meta.m.commits, total, L.hrows.d, G.d_grows, L.stream);
    WZCHK(merge_tail(e, L, c, y.most, G.d_grows));
    // 5. the state the commit launch leaves behind, and what wz_gate_stats reports
    G.g_ran.assign(n, 0);
    G.g_act.assign(act, act + total);
    G.g_tiles = total; G.g_crows = crows; G.g_cols = cols; G.g_masked = masked;
    k = 0;
    for (int i = 0; i < n; ++i) {
        GateCam& g = *cams[i];
        g.lane = slot;
        for (int t = 0; t < nt[i]; ++t, ++k) {
            if (runs[k]) {
                g.has_ref[t] = 1;
                g.skipped[t] = 0;
                G.g_ran[i] |= 1ull << t;
            } else {
                ++g.skipped[t];
            }
        }
    }
    return WZ_OK;
}


// ---- motion regions: whole-frame activity launch -> region launch -> the host reads the rectangles -> a tiled call on them (k_motion.hip,
// DESIGN.md section 19)
// Why these settings are refused for a w x h frame of format word fmt (wz_last_error is set), or WZ_OK; e null: the engine's limits are not looked at
static int motion_refusal(const wz_engine* e, const char* who, int w, int h, int fmt, const wz_motion_t& p) {
    if (!wz_frame_bytes(w, h, fmt)) return wz_set_error(WZ_EINVAL, "%s: pixel format 0x%x at %dx%d: %s", who, fmt, w, h, fmt_refusal(w, h, fmt));
    if (p.pixel_thr < 0 || p.pixel_thr > 255 || p.min_cells < 1 || p.dilate < 0 || p.dilate > 2 || p.max_regions < 1 || p.max_regions > WZ_MOTION_MAX_REGIONS ||
        p.min_side < WZ_GATE_CELL || p.pad < 0 || p.pad > 64 || (p.whole_frame != 0 && p.whole_frame != 1))
        return wz_set_error(WZ_EINVAL, "%s: motion (%d, %d, %d, %d, %d, %d, %d): pixel_thr must be 0 .. 255, min_cells >= 1, dilate 0 .. 2, max_regions 1 .. %d, "
                            "min_side >= %d, pad 0 .. 64, whole_frame 0 or 1", who, p.pixel_thr, p.min_cells, p.dilate, p.max_regions, p.min_side, p.pad,
                            p.whole_frame, WZ_MOTION_MAX_REGIONS, WZ_GATE_CELL);
    if (e && (w > e->max_w || h > e->max_h || (size_t)w * h * 3 > e->frame_stride))
        return wz_set_error(WZ_ELIMIT, "%s: the frame is %dx%d, engine was created for at most %dx%d", who, w, h, e->max_w, e->max_h);
    if (gate_cells_of(w, h) > (size_t)WZ_MOTION_MAX_CELLS)
        return wz_set_error(WZ_ELIMIT, "%s: a %dx%d frame has %zu cells, a motion camera takes at most %d", who, w, h, gate_cells_of(w, h), WZ_MOTION_MAX_CELLS);
    if (e && p.whole_frame + p.max_regions > e->max_batch)
        return wz_set_error(WZ_ELIMIT, "%s: whole_frame + max_regions = %d tiles exceed max_batch %d", who, p.whole_frame + p.max_regions, e->max_batch);
    return WZ_OK;
}

// what the region kernel gets for a w x h frame of format word fmt
static void motion_desc(int w, int h, int fmt, const wz_motion_t& p, const uint16_t* now, const uint16_t* ref, uint32_t* scratch, WzMotionCam& d) {
    const int base = fmt & WZ_FMT_BASE_MASK;
    const bool planar = base == WZ_FMT_NV12 || base == WZ_FMT_I420 || base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10;
    d.now = now; d.ref = ref; d.scratch = scratch;
    d.W = w; d.H = h;
    d.gw = cells_of(w);
    d.gh = cells_of(h);
    d.thr = p.pixel_thr; d.min_cells = p.min_cells; d.dilate = p.dilate; d.max_regions = p.max_regions; d.min_side = p.min_side; d.pad = p.pad;
    d.even_x = (planar || base == WZ_FMT_YUYV422 || base == WZ_FMT_UYVY422) ? 1 : 0;
    d.even_y = planar ? 1 : 0;
    d.age_in = nullptr; d.age_out = nullptr;   // (no hold; motion_hold_desc adds one)
    d.hold = d.object_hold = 0;
    d.ignore = nullptr;                        // (no mask; a camera with one adds its bits)
}
// ... and of a camera with a hold on top of it: the ages it reads (null: all zero) and the grid that takes the ages it leaves
static void motion_hold_desc(const uint8_t* age_in, uint8_t* age_out, int hold, int object_hold, WzMotionCam& d) {
    d.age_in = age_in; d.age_out = age_out;
    d.hold = hold; d.object_hold = object_hold;
}

// A checked motion call on a drained lane, frames in device memory.  Returns once the rectangles are read: the two launches that touch the
// cameras' luma grids have finished by then; crop, batch, merge and filters are enqueued behind, and the lane's event behind them.  No
// other lane can hold the motion state of a camera WITHOUT a hold in flight.  A camera with one has its stamp launch -- the last of the
// call, behind the filters -- in flight when this returns: its next call on another lane waits for this lane first, as a gated call does.
static int motion_enqueue(wz_engine* e, int slot, const TileCall& call) {
    Lane& L = e->lanes[slot];
    MotionLane& M = L.motion;
    WZCHK(L.tile.alloc(e));
    WZCHK(M.alloc(e));
    const int n = call.n;
    constexpr int PER = 1 + WZ_MOTION_MAX_REGIONS;
    const std::vector<MotionCam*> cams = cams_of(e->motion_cams, call);
    // 1. the whole frame's grid of every camera, one launch; 2. its regions, one launch; then the one wait of the call
    WzGateTile* gt = M.meta.h.tiles;
    WzMotionCam* md = M.meta.h.cams;
    WzMotionOut* mo = M.meta.h.outs;
    int crows = 0, cols = 0, cells = 0;
    bool aged = false, stamps = false;   // some camera of the call has a hold; ... and holds under detections
    bool masked = false;                 // some camera of the call has an ignore mask
    for (const MotionCam* m : cams)      // another lane's stamp launch may still be writing this camera's ages
        if (m->d_age[0] && m->lane >= 0 && m->lane != slot) HIPCHK(hipEventSynchronize(e->lanes[m->lane].done));
    for (int i = 0; i < n; ++i) {
        MotionCam& m = *cams[i];
        const wz_tile_t whole = {0, 0, m.w, m.h};
        uint16_t* now = m.d_grid[m.cur ^ 1];
        gate_tile(call.frames[i], m.w, call.pf(i), whole, gt[i]);
        gt[i].ref = nullptr;   // (the region launch compares: this launch only sums)
        gt[i].now = now;
        gt[i].thr = 0;
        motion_desc(m.w, m.h, call.pf(i), m.p, now, m.has_ref ? m.d_grid[m.cur].p : nullptr, M.d_mscratch + M.cam_words * i, md[i]);
        if (m.d_age[0]) {
            motion_hold_desc(m.has_age ? m.d_age[m.cur].p : nullptr, m.d_age[m.cur ^ 1], m.hold, m.object_hold, md[i]);
            aged = true;
            stamps = stamps || m.object_hold > 0;
        }
        if (m.d_ignore) {
            md[i].ignore = m.d_ignore;
            masked = true;
        }
        crows = std::max(crows, gt[i].crows);
        cols = std::max(cols, gt[i].cols);
        cells = std::max(cells, m.gw * m.gh);
        mo[i].n_regions = -1;
    }
    wz_launch_tile_activity(M.meta.m.tiles, n, crows, cols, M.d_mcount, M.meta.m.activity, L.stream);
    wz_launch_motion_regions(M.meta.m.cams, n, cells, M.meta.m.outs, L.stream, aged, masked);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(L.stream));   // the batch size is a host-side quantity: the plan waits for the rectangles
    // 3. the tile lists; the cameras' state changes only once everything is enqueued
    std::vector<wz_tile_t> tiles((size_t)n * PER);
    std::vector<int32_t> nt(n), comps(n), ncell((size_t)n * WZ_MOTION_MAX_REGIONS, 0), active(n), held(n), ignored(n);
    std::vector<const wz_tile_t*> tp(n);
    bool still = false;
    for (int i = 0; i < n; ++i) {
        const MotionCam& m = *cams[i];
        const WzMotionOut& o = mo[i];
        if (o.n_regions < 0 || o.n_regions > m.p.max_regions) return wz_set_error(WZ_EHIP, "frame %d: the region launch reported %d regions", i, o.n_regions);
        wz_tile_t* t = &tiles[(size_t)i * PER];
        int k = 0;
        if (m.p.whole_frame) t[k++] = {0, 0, m.w, m.h};
        for (int r = 0; r < o.n_regions; ++r, ++k) {
            t[k] = o.regions[r];
            ncell[(size_t)i * WZ_MOTION_MAX_REGIONS + r] = o.cells[r];
        }
        for (int j = 0; j < k; ++j) WZCHK(tile_fits(e, "frame", i, m.w, m.h, call.pf(i), j, t[j]));
        nt[i] = k;
        tp[i] = t;
        comps[i] = o.components;
        active[i] = o.active;
        held[i] = o.held;
        ignored[i] = o.ignored;
        still = still || k == 0;
    }
    const TileCall c = with_tiles(call, nt, tp);   // ... a tiled call on these lists
    TilePlan y;
    tile_plan(e, L, c, nullptr, y);
    WZCHK(run_tiles(e, slot, y));
    WZCHK(merge_tail(e, L, c, y.most, L.hrows.d, still, stamps ? M.meta.m.cams : nullptr));
    // 4. the grids this call wrote are the next call's reference and ages; what wz_motion_stats, wz_motion_hold_stats and
    // wz_motion_ignore_stats report
    for (int i = 0; i < n; ++i) {
        cams[i]->cur ^= 1;
        cams[i]->has_ref = true;
        if (cams[i]->d_age[0]) {
            cams[i]->has_age = true;
            cams[i]->lane = slot;
        }
    }
    M.s_ntiles.swap(nt);
    M.s_tiles.swap(tiles);
    M.s_cells.swap(ncell);
    M.s_comps.swap(comps);
    M.s_active.swap(active);
    M.s_held.swap(held);
    M.s_ignored.swap(ignored);
    return WZ_OK;
}

// ---- the entry points of the three kinds
enum { KIND_TILED = 0, KIND_GATED = 1, KIND_MOTION = 2 };
static int enqueue(wz_engine* e, int slot, const TileCall& c, int kind) {
    return kind == KIND_MOTION ? motion_enqueue(e, slot, c) : kind == KIND_GATED ? gated_enqueue(e, slot, c) : tiled_enqueue(e, slot, c);
}

// a checked call of frames in device memory, on its lane once the lane's previous batch has fully drained
static int submit_device(wz_engine* e, int slot, const TileCall& c, int kind) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->lanes[slot].done));
    return enqueue(e, slot, c, kind);
}

// a checked call of host frames on lane 0, start to rows: every frame whole into the lane's staging area, as wz_submit_host_fmt stages it
// (the tiles are cut from that copy), enqueue, collect, the wall time into ms
static int detect_staged(wz_engine* e, TileCall& c, int kind, wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(e->device));
    Lane& L = e->lanes[0];
    HIPCHK(hipEventSynchronize(L.done));
    std::vector<const uint8_t*> dptr(c.n);
    for (int i = 0; i < c.n; ++i) WZCHK(stage_frame(e, L, i, c.frames[i], wz_frame_bytes(c.w[i], c.h[i], c.pf(i)), &dptr[i]));
    c.frames = dptr.data();
    WZCHK(enqueue(e, 0, c, kind));
    return collect_timed(e, c.n, out, pass, ms, t0);   // WZ_OK, or WZ_EINCOMPLETE: the merged rows are written, the rows of a tile that ran in this call may have been short
}

extern "C" int wz_submit_tiled_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h,
                                      const int* fmt, const int* cam, const int* n_tiles, const wz_tile_t* const* tiles,
                                      double iou_thr, double ios_thr) {
    TileCall c = {n, d_frames, w, h, fmt, cam, n_tiles, tiles, iou_thr, ios_thr, 0};
    WZCHK(tiled_check(e, "wz_submit_tiled_device", slot, c, false));
    return submit_device(e, slot, c, KIND_TILED);
}
extern "C" int wz_detect_tiled(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt,
                               const int* cam, const int* n_tiles, const wz_tile_t* const* tiles, double iou_thr, double ios_thr,
                               wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    TileCall c = {n, frames, w, h, fmt, cam, n_tiles, tiles, iou_thr, ios_thr, 0};
    WZCHK(tiled_check(e, "wz_detect_tiled", 0, c, true));
    return detect_staged(e, c, KIND_TILED, out, pass, ms);
}
extern "C" int wz_submit_gated_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                                      const int* cam, double iou_thr, double ios_thr) {
    TileCall c = {n, d_frames, w, h, fmt, cam, nullptr, nullptr, iou_thr, ios_thr, 0};
    WZCHK(camera_check(e, &wz_engine::gate_cams, GATED, "wz_submit_gated_device", slot, c, false));
    return submit_device(e, slot, c, KIND_GATED);
}
extern "C" int wz_detect_gated(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt, const int* cam,
                               double iou_thr, double ios_thr, wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    TileCall c = {n, frames, w, h, fmt, cam, nullptr, nullptr, iou_thr, ios_thr, 0};
    WZCHK(camera_check(e, &wz_engine::gate_cams, GATED, "wz_detect_gated", 0, c, true));
    return detect_staged(e, c, KIND_GATED, out, pass, ms);
}

extern "C" int wz_gate_stats(wz_engine_t* e, int slot, int n, uint64_t* ran_mask, int32_t* activity) {
    if (!e || !ran_mask || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_gate_stats: bad argument");
    const GateLane& G = e->lanes[slot].gate;
    if (n < 1 || n != (int)G.g_ran.size())
        return wz_set_error(WZ_EINVAL, "wz_gate_stats: the last gated call on lane %d had %d frames, not %d", slot, (int)G.g_ran.size(), n);
    memcpy(ran_mask, G.g_ran.data(), sizeof(uint64_t) * n);
    if (activity) memcpy(activity, G.g_act.data(), sizeof(int32_t) * G.g_act.size());
    return WZ_OK;
}


// ---- a camera's motion settings, and the motion calls
extern "C" int wz_set_camera_motion(wz_engine_t* e, int cam, int width, int height, int fmt, const wz_motion_t* motion) {
    if (!e || !motion) return wz_set_error(WZ_EINVAL, "wz_set_camera_motion: null argument");
    if (cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_ELIMIT, "camera id %d out of range [0,%d)", cam, WZ_MAX_CAMS);
    char who[48];
    snprintf(who, sizeof who, "camera %d", cam);
    WZCHK(motion_refusal(e, who, width, height, fmt, *motion));
    MotionCam m;
    m.w = width; m.h = height; m.fmt = fmt; m.base = fmt & WZ_FMT_BASE_MASK;
    m.gw = cells_of(width);
    m.gh = cells_of(height);
    m.p = *motion;
    m.p._reserved = 0;
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    // the new grids are allocated aside: a failure leaves the camera with the settings (and the reference) it had
    hipError_t err = m.d_grid[0].alloc((size_t)m.gw * m.gh);
    if (err == hipSuccess) err = m.d_grid[1].alloc((size_t)m.gw * m.gh);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_set_camera_motion: %s (camera %d keeps its previous settings)", hipGetErrorString(err), cam);
    e->motion_cams[cam] = std::move(m);   // (m leaves with the old grids: nothing in flight reads them, every lane was synchronised above)
    return WZ_OK;
}

extern "C" int wz_reset_camera_motion(wz_engine_t* e, int cam) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_reset_camera_motion: null engine");
    auto it = e->motion_cams.find(cam);
    if (it == e->motion_cams.end()) return wz_set_error(WZ_EINVAL, "camera %d has no motion settings (wz_set_camera_motion first)", cam);
    it->second.has_ref = false;   // (a motion call leaves no launch in flight that reads the grids: nothing to wait for)
    it->second.has_age = false;   // (a stamp launch in flight writes a grid nobody reads any more; the camera's next call is ordered behind it)
    return WZ_OK;
}

// A camera's hold: its two age grids, allocated aside behind sync_all -- a failure leaves the camera with what it had
extern "C" int wz_set_camera_motion_hold(wz_engine_t* e, int cam, const wz_motion_hold_t* hold) {
    if (!e || !hold) return wz_set_error(WZ_EINVAL, "wz_set_camera_motion_hold: null argument");
    auto it = e->motion_cams.find(cam);
    if (it == e->motion_cams.end()) return wz_set_error(WZ_EINVAL, "camera %d has no motion settings (wz_set_camera_motion first, then its hold)", cam);
    if (hold->hold < 0 || hold->hold > 255 || hold->object_hold < 0 || hold->object_hold > 255)
        return wz_set_error(WZ_EINVAL, "camera %d: motion hold (%d, %d): hold and object_hold must be 0 .. 255", cam, hold->hold, hold->object_hold);
    MotionCam& m = it->second;
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    DevBlock<uint8_t> age[2];   // (both 0: the camera's grids leave with these two, empty)
    if (hold->hold || hold->object_hold) {
        hipError_t err = age[0].alloc((size_t)m.gw * m.gh);
        if (err == hipSuccess) err = age[1].alloc((size_t)m.gw * m.gh);
        if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_set_camera_motion_hold: %s (camera %d keeps its previous hold)", hipGetErrorString(err), cam);
    }
    m.d_age[0] = std::move(age[0]);
    m.d_age[1] = std::move(age[1]);
    m.hold = hold->hold;
    m.object_hold = hold->object_hold;
    m.has_age = false;
    m.lane = -1;
    return WZ_OK;
}

extern "C" int wz_clear_camera_motion(wz_engine_t* e, int cam) {
    if (!e || cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_EINVAL, "wz_clear_camera_motion: bad argument");
    auto it = e->motion_cams.find(cam);
    if (it == e->motion_cams.end()) return WZ_OK;
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    e->motion_cams.erase(it);
    return WZ_OK;
}

extern "C" int wz_submit_motion_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                                       const int* cam, double iou_thr, double ios_thr) {
    TileCall c = {n, d_frames, w, h, fmt, cam, nullptr, nullptr, iou_thr, ios_thr, 0};
    WZCHK(camera_check(e, &wz_engine::motion_cams, MOTION, "wz_submit_motion_device", slot, c, false));
    return submit_device(e, slot, c, KIND_MOTION);
}
extern "C" int wz_detect_motion(wz_engine_t* e, int n, const uint8_t* const* frames, const int* w, const int* h, const int* fmt, const int* cam,
                                double iou_thr, double ios_thr, wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    TileCall c = {n, frames, w, h, fmt, cam, nullptr, nullptr, iou_thr, ios_thr, 0};
    WZCHK(camera_check(e, &wz_engine::motion_cams, MOTION, "wz_detect_motion", 0, c, true));
    return detect_staged(e, c, KIND_MOTION, out, pass, ms);
}

extern "C" int wz_motion_stats(wz_engine_t* e, int slot, int n, int32_t* n_tiles, wz_tile_t* tiles, int32_t* cells, int32_t* components) {
    if (!e || !n_tiles || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_motion_stats: bad argument");
    const MotionLane& M = e->lanes[slot].motion;
    if (n < 1 || n != (int)M.s_ntiles.size())
        return wz_set_error(WZ_EINVAL, "wz_motion_stats: the last motion call on lane %d had %d frames, not %d", slot, (int)M.s_ntiles.size(), n);
    memcpy(n_tiles, M.s_ntiles.data(), sizeof(int32_t) * n);
    if (tiles) memcpy(tiles, M.s_tiles.data(), sizeof(wz_tile_t) * M.s_tiles.size());
    if (cells) memcpy(cells, M.s_cells.data(), sizeof(int32_t) * M.s_cells.size());
    if (components) memcpy(components, M.s_comps.data(), sizeof(int32_t) * n);
    return WZ_OK;
}

extern "C" int wz_motion_hold_stats(wz_engine_t* e, int slot, int n, int32_t* active, int32_t* held) {
    if (!e || !active || !held || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_motion_hold_stats: bad argument");
    const MotionLane& M = e->lanes[slot].motion;
    if (n < 1 || n != (int)M.s_active.size())
        return wz_set_error(WZ_EINVAL, "wz_motion_hold_stats: the last motion call on lane %d had %d frames, not %d", slot, (int)M.s_active.size(), n);
    memcpy(active, M.s_active.data(), sizeof(int32_t) * n);
    memcpy(held, M.s_held.data(), sizeof(int32_t) * n);
    return WZ_OK;
}

extern "C" int wz_motion_ignore_stats(wz_engine_t* e, int slot, int n, int32_t* ignored) {
    if (!e || !ignored || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_motion_ignore_stats: bad argument");
    const MotionLane& M = e->lanes[slot].motion;
    if (n < 1 || n != (int)M.s_ignored.size())
        return wz_set_error(WZ_EINVAL, "wz_motion_ignore_stats: the last motion call on lane %d had %d frames, not %d", slot, (int)M.s_ignored.size(), n);
    memcpy(ignored, M.s_ignored.data(), sizeof(int32_t) * n);
    return WZ_OK;
}

// ---- a camera's ignore mask: the cell bits of the frame's grid for its motion settings, of every tile's own grid
// for its gate layout.  Built aside behind sync_all: a failure leaves the camera with what it had
extern "C" int wz_set_camera_ignore(wz_engine_t* e, int cam, int width, int height, const uint8_t* ignore) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_set_camera_ignore: null engine");
    const auto mi = e->motion_cams.find(cam);
    const auto gi = e->gate_cams.find(cam);
    MotionCam* m = mi == e->motion_cams.end() ? nullptr : &mi->second;
    GateCam* g = gi == e->gate_cams.end() ? nullptr : &gi->second;
    if (!m && !g)
        return wz_set_error(WZ_EINVAL, "camera %d has neither motion settings nor tiles: an ignore mask is set after wz_set_camera_motion / wz_set_camera_tiles", cam);
    HIPCHK(hipSetDevice(e->device));
    if (!ignore) {   // remove
        WZCHK(sync_all(e));
        if (m) m->d_ignore = DevBlock<unsigned long long>();
        if (g) g->d_ignore = DevBlock<uint32_t>(), g->ignore_off.clear();
        return WZ_OK;
    }
    if (m && (width != m->w || height != m->h))
        return wz_set_error(WZ_EINVAL, "camera %d: the ignore plane is %dx%d but the camera's motion settings were made for %dx%d", cam, width, height, m->w, m->h);
    if (g && (width != g->w || height != g->h))
        return wz_set_error(WZ_EINVAL, "camera %d: the ignore plane is %dx%d but the camera's tiles were set for %dx%d", cam, width, height, g->w, g->h);
    WZCHK(sync_all(e));
    std::vector<uint8_t> cells;
    std::vector<unsigned long long> words;
    DevBlock<unsigned long long> d_motion;
    DevBlock<uint32_t> d_gate;
    std::vector<size_t> off;
    hipError_t err = hipSuccess;
    if (m) {
        const size_t n = (size_t)m->gw * m->gh;
        cells.resize(n);
        words.resize(ignore_words_of(n));
        if (wz_ignore_cells(ignore, width, height, nullptr, cells.data()) != WZ_OK) return wz_set_error(WZ_EINVAL, "wz_set_camera_ignore: bad plane");
        pack_cell_bits(cells.data(), n, words.data());
        err = d_motion.alloc(words.size());
        if (err == hipSuccess) err = hipMemcpy(d_motion, words.data(), words.size() * 8, hipMemcpyHostToDevice);
    }
    if (g && err == hipSuccess) {
        words.clear();
        for (size_t t = 0; t < g->tiles.size(); ++t) {   // (every tile's bits begin at a 64-bit word)
            const size_t n = (size_t)g->cols[t] * g->crows[t], at = words.size();
            cells.resize(n);
            words.resize(at + ignore_words_of(n));
            if (wz_ignore_cells(ignore, width, height, &g->tiles[t], cells.data()) != WZ_OK) return wz_set_error(WZ_EINVAL, "wz_set_camera_ignore: bad plane");
            pack_cell_bits(cells.data(), n, words.data() + at);
            off.push_back(2 * at);
        }
        err = d_gate.alloc(2 * words.size());
        if (err == hipSuccess) err = hipMemcpy(d_gate, words.data(), words.size() * 8, hipMemcpyHostToDevice);
    }
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_set_camera_ignore: %s (camera %d keeps its previous mask)", hipGetErrorString(err), cam);
    if (m) m->d_ignore = std::move(d_motion);   // (the old bits leave with these two: nothing in flight reads them, every lane was synchronised above)
    if (g) g->d_ignore = std::move(d_gate), g->ignore_off.swap(off);
    return WZ_OK;
}

// ---- a camera's layout and gate
extern "C" int wz_set_camera_tiles(wz_engine_t* e, int cam, int width, int height, int fmt, int n_tiles, const wz_tile_t* tiles,
                                   const wz_tile_gate_t* gate) {
    if (!e || !tiles || !gate) return wz_set_error(WZ_EINVAL, "wz_set_camera_tiles: null argument");
    if (cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_ELIMIT, "camera id %d out of range [0,%d)", cam, WZ_MAX_CAMS);
    if (!wz_frame_bytes(width, height, fmt))
        return wz_set_error(WZ_EINVAL, "camera %d: pixel format 0x%x at %dx%d: %s", cam, fmt, width, height, fmt_refusal(width, height, fmt));
    if (n_tiles < 1 || n_tiles > WZ_MAX_TILES) return wz_set_error(WZ_ELIMIT, "camera %d: %d tiles, a frame takes 1 to %d", cam, n_tiles, WZ_MAX_TILES);
    if (n_tiles > e->max_batch) return wz_set_error(WZ_ELIMIT, "camera %d: %d tiles exceed max_batch %d", cam, n_tiles, e->max_batch);
    if (gate->pixel_thr < 0 || gate->pixel_thr > 255 || gate->min_cells < 1 || gate->max_age < 0)
        return wz_set_error(WZ_EINVAL, "camera %d: gate (%d, %d, %d): pixel_thr must be 0 .. 255, min_cells >= 1, max_age >= 0", cam, gate->pixel_thr,
                            gate->min_cells, gate->max_age);
    GateCam g;
    g.w = width; g.h = height; g.base = fmt & WZ_FMT_BASE_MASK;
    g.gate = *gate;
    g.gate._reserved = 0;
    size_t cells = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const wz_tile_t& r = tiles[t];
        WZCHK(tile_fits(e, "camera", cam, width, height, fmt, t, r));
        g.tiles.push_back(r);
        g.cols.push_back(cells_of(r.w));
        g.crows.push_back(cells_of(r.h));
        g.grid_off.push_back(cells);
        cells += (gate_cells_of(r.w, r.h) + 7) & ~(size_t)7;   // (every grid begins at a 16-byte boundary)
    }
    g.has_ref.assign(n_tiles, 0);
    g.skipped.assign(n_tiles, 0);
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    // the new state is allocated aside: a failure leaves the camera with the layout (and the references) it had
    hipError_t err = g.d_ref.alloc(cells);
    if (err == hipSuccess) err = g.d_rows.alloc((size_t)WZ_MAX_DETECTIONS * n_tiles);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_set_camera_tiles: %s (camera %d keeps its previous tiles)", hipGetErrorString(err), cam);
    e->gate_cams[cam] = std::move(g);   // (g leaves with the old state: nothing in flight reads it, every lane was synchronised above)
    return WZ_OK;
}

extern "C" int wz_reset_camera_tiles(wz_engine_t* e, int cam) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_reset_camera_tiles: null engine");
    auto it = e->gate_cams.find(cam);
    if (it == e->gate_cams.end()) return wz_set_error(WZ_EINVAL, "camera %d has no tiles (wz_set_camera_tiles first)", cam);
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    std::fill(it->second.has_ref.begin(), it->second.has_ref.end(), (uint8_t)0);
    std::fill(it->second.skipped.begin(), it->second.skipped.end(), 0);
    return WZ_OK;
}

extern "C" int wz_clear_camera_tiles(wz_engine_t* e, int cam) {
    if (!e || cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_EINVAL, "wz_clear_camera_tiles: bad argument");
    auto it = e->gate_cams.find(cam);
    if (it == e->gate_cams.end()) return WZ_OK;
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    e->gate_cams.erase(it);
    return WZ_OK;
}

// ---- the frame table's tiled entries
// Entries first .. first + count - 1 get a tiled description (include/watsor_hip.h); checked against every entry as tiled_check checks a
// call, nothing changes on a refusal.
extern "C" int wz_bind_tiles(wz_engine_t* e, int first, int count, int n_tiles, const wz_tile_t* tiles, double iou_thr, double ios_thr, int gated) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_bind_tiles: null engine");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));   // no batch in flight was planned with the old descriptions
    const int64_t size = (int64_t)e->bound.size();
    if (first < 0 || count < 1 || (int64_t)first + count > size)
        return wz_set_error(WZ_EINVAL, "wz_bind_tiles: entries %d .. %lld lie outside the frame table of %lld entries", first, (long long)first + count - 1,
                            (long long)size);
    wz_engine::BoundTiles d;
    if (gated) {
        if (tiles || n_tiles != 0)
            return wz_set_error(WZ_EINVAL, "wz_bind_tiles: a gated description takes its %d rectangles from wz_set_camera_tiles: tiles must be NULL and n_tiles 0", n_tiles);
        const int c = e->bound[first].cam;
        for (int i = first; i < first + count; ++i)
            if (e->bound[i].cam < 0 || e->bound[i].cam != c)
                return wz_set_error(WZ_EINVAL, "wz_bind_tiles: gated entries %d .. %d must carry one camera id >= 0, entry %d has %d and entry %d has %d", first,
                                    first + count - 1, first, c, i, e->bound[i].cam);
        d.kind = wz_engine::BOUND_GATED;
    } else if (n_tiles == 0 && !tiles) {
        d.kind = wz_engine::BOUND_PLAIN;
    } else {
        const int most = std::min(WZ_MAX_TILES, e->max_batch);
        if (n_tiles < 1 || n_tiles > most) return wz_set_error(WZ_ELIMIT, "wz_bind_tiles: %d tiles, an entry of this engine takes 1 to %d", n_tiles, most);
        if (!tiles) return wz_set_error(WZ_EINVAL, "wz_bind_tiles: %d tiles but no rectangles", n_tiles);
        for (int i = first; i < first + count; ++i)
            for (int t = 0; t < n_tiles; ++t) {
                const wz_engine::BoundFrame& f = e->bound[i];
                WZCHK(tile_fits(e, "frame-table entry", i, f.w, f.h, f.fmt, t, tiles[t]));
            }
        d.kind = wz_engine::BOUND_TILED;
        d.tiles.assign(tiles, tiles + n_tiles);
    }
    if (d.kind != wz_engine::BOUND_PLAIN) {
        if (!(iou_thr >= 0.0) || !(ios_thr >= 0.0)) return wz_set_error(WZ_EINVAL, "wz_bind_tiles: the merge thresholds (%g, %g) must be numbers >= 0", iou_thr, ios_thr);
        d.iou = iou_thr;
        d.ios = ios_thr;
        if (e->bound_tiles.empty()) e->bound_tiles.resize(e->bound.size());
    }
    if (e->bound_tiles.empty()) return WZ_OK;   // (untiled entries of a table without descriptions)
    for (int i = first; i < first + count; ++i) e->bound_tiles[i] = d;
    bool any = false;
    for (const auto& b : e->bound_tiles) any = any || b.kind != wz_engine::BOUND_PLAIN;
    if (!any) e->bound_tiles.clear();
    return WZ_OK;
}

// ---- the frame table's motion entries
// Entries first .. first + count - 1 get a motion description (include/watsor_hip.h): the thresholds and nothing else -- the camera's
// settings, hold and mask are looked up at every submit, as a gated description looks up its layout.  Nothing changes on a refusal.
extern "C" int wz_bind_motion(wz_engine_t* e, int first, int count, double iou_thr, double ios_thr) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_bind_motion: null engine");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));   // no batch in flight was planned with the old descriptions
    const int64_t size = (int64_t)e->bound.size();
    if (first < 0 || count < 1 || (int64_t)first + count > size)
        return wz_set_error(WZ_EINVAL, "wz_bind_motion: entries %d .. %lld lie outside the frame table of %lld entries", first, (long long)first + count - 1,
                            (long long)size);
    const int c = e->bound[first].cam;
    for (int i = first; i < first + count; ++i)
        if (e->bound[i].cam < 0 || e->bound[i].cam != c)
            return wz_set_error(WZ_EINVAL, "wz_bind_motion: motion entries %d .. %d must carry one camera id >= 0, entry %d has %d and entry %d has %d", first,
                                first + count - 1, first, c, i, e->bound[i].cam);
    if (!(iou_thr >= 0.0) || !(ios_thr >= 0.0)) return wz_set_error(WZ_EINVAL, "wz_bind_motion: the merge thresholds (%g, %g) must be numbers >= 0", iou_thr, ios_thr);
    wz_engine::BoundTiles d;
    d.kind = wz_engine::BOUND_MOTION;
    d.iou = iou_thr;
    d.ios = ios_thr;
    if (e->bound_tiles.empty()) e->bound_tiles.resize(e->bound.size());
    for (int i = first; i < first + count; ++i) e->bound_tiles[i] = d;
    return WZ_OK;
}

// The bytes the crop kernel (and, gated, the activity kernel before it) reads of a frame: what decides between reading a page-locked frame in
// place and staging it whole.  Break-even by bandwidth is near 0.8 of the frame's bytes (a kernel reads mapped memory at 23 GB/s beside the
// other lanes' kernels, the copies move 29 GB/s: see stage_frame in wz_engine.hip); one half is the margin read_in_place() uses for the resize kernel.
// Measured for the crop kernel (profiles/bound_tiles.txt; one 640 x 480 rectangle of a 1080p frame, four lanes busy):
// RGB24, cost 0.15 of the frame: 5600 frames/s in place against 5565 staged -- level -- and a lone call 0.326 against 0.426 ms; NV12, cost
// 0.15: 5825 in place against 8247 staged, a lone call 0.318 against 0.374 ms.  So at a cost well under one half, reading in place is
// SLOWER than staging with every lane busy once the whole frame is small (3.1 MB): both in-place legs sit at ~0.175 ms a step whatever
// they read.  The constant stays at one half here; moving it (or bounding it by the frame's bytes) needs that plateau explained first.
// A MOTION entry never comes here and host_read is not consulted for it: its activity launch reads every luma pixel of the frame -- at
// least 2/3 of an NV12 frame's bytes, all of an RGB24 frame's -- before any rectangle is cut, so its cost can never be at most half the
// frame, and the in-place leg measured slower than staging with every lane busy even far below that.  It is always staged whole.
static bool tiles_in_place(const wz_engine* e, const wz_engine::BoundFrame& f, const std::vector<wz_tile_t>& tiles, bool gated) {
    if (!f.dev || e->host_read == 0) return false;
    if (e->host_read == 1) return true;
    uint64_t cost = 0;
    for (const wz_tile_t& t : tiles) cost += wz_frame_bytes(t.w, t.h, f.fmt);
    if (gated) cost *= 2;   // a gated tile is measured, and read again when it runs
    return e->host_read == 2 && 2 * cost <= f.bytes;
}

static const char* bound_kind_name(int kind) {
    return kind == wz_engine::BOUND_TILED ? "tiled" : kind == wz_engine::BOUND_GATED ? "gated" : kind == wz_engine::BOUND_MOTION ? "motion" : "untiled";
}

// wz_submit_bound of a batch with a tiled, gated or motion entry (slot, n and the entries' range are checked): one kind, one pair of
// thresholds, the refusals of the tiled / gated / motion call, then every frame staged whole or (tiled, gated) handed over in place, then
// tiled_enqueue / gated_enqueue / motion_enqueue.
int submit_bound_tiles(wz_engine* e, int slot, int n, const int32_t* entries) {
    const wz_engine::BoundTiles& d0 = e->bound_tiles[entries[0]];
    for (int i = 1; i < n; ++i) {
        const wz_engine::BoundTiles& d = e->bound_tiles[entries[i]];
        if (d.kind != d0.kind)
            return wz_set_error(WZ_EINVAL, "wz_submit_bound: frame-table entry %d is %s and entry %d is %s: a batch holds one kind", entries[0],
                                bound_kind_name(d0.kind), entries[i], bound_kind_name(d.kind));
    }
    for (int i = 1; i < n; ++i) {
        const wz_engine::BoundTiles& d = e->bound_tiles[entries[i]];
        if (d.iou != d0.iou || d.ios != d0.ios)
            return wz_set_error(WZ_EINVAL, "wz_submit_bound: frame-table entry %d merges with thresholds (%g, %g) and entry %d with (%g, %g): a batch takes one pair",
                                entries[0], d0.iou, d0.ios, entries[i], d.iou, d.ios);
    }
    const bool gated = d0.kind == wz_engine::BOUND_GATED, motion = d0.kind == wz_engine::BOUND_MOTION;
    BoundBatch b;
    bound_gather(e, n, entries, b);
    std::vector<int> nt(n);
    std::vector<const wz_tile_t*> tp(n);
    for (int i = 0; i < n; ++i) {
        nt[i] = (int)e->bound_tiles[entries[i]].tiles.size();
        tp[i] = e->bound_tiles[entries[i]].tiles.data();
    }
    TileCall c = {n, b.ptr.data(), b.w, b.h, b.fmt, b.cam, nt.data(), tp.data(), d0.iou, d0.ios, 0};
    WZCHK(motion  ? camera_check(e, &wz_engine::motion_cams, MOTION, "wz_submit_bound", slot, c, true)
          : gated ? camera_check(e, &wz_engine::gate_cams, GATED, "wz_submit_bound", slot, c, true)
                  : tiled_check(e, "wz_submit_bound", slot, c, true));
    WZCHK(bound_drain(e, slot));
    Lane& L = e->lanes[slot];
    std::vector<int32_t> src(n);
    for (int i = 0; i < n; ++i) {
        const wz_engine::BoundFrame& f = e->bound[entries[i]];
        if (!motion) {   // (a motion entry has no in-place leg: see tiles_in_place)
            const std::vector<wz_tile_t>& tiles = gated ? e->gate_cams.find(f.cam)->second.tiles : e->bound_tiles[entries[i]].tiles;
            if (tiles_in_place(e, f, tiles, gated)) {
                b.ptr[i] = f.dev;
                src[i] = 1;
                continue;
            }
        }
        WZCHK(stage_frame(e, L, i, f.host, f.bytes, &b.ptr[i]));
    }
    WZCHK(enqueue(e, slot, c, motion ? KIND_MOTION : gated ? KIND_GATED : KIND_TILED));
    L.bound_idx.assign(entries, entries + n);   // (L.tile.tiled == n says that their rows are the merged ones)
    L.bound_src.swap(src);
    return WZ_OK;
}

#ifdef WZ_DEV_BUILD   // ---- everything below this line exists in libwatsor_hip_dev.so only (include/watsor_hip.h, last section)
// ---- stage-level entry points (parity tests) and profiling
// One rectangle of one host frame for a kernel of its own: the checks, then a device copy of the frame that starts at the host pointer's
// offset within 16 bytes, so that what a caller does to the source's alignment reaches the kernel.  *base is what to free.
static int one_tile_check(int w, int h, int fmt, const wz_tile_t* tile) {
    if (!wz_frame_bytes(w, h, fmt)) return wz_set_error(WZ_EINVAL, "pixel format 0x%x at %dx%d: %s", fmt, w, h, fmt_refusal(w, h, fmt));
    const char* why = tile_refusal(*tile, w, h, fmt);
    if (why) return wz_set_error(WZ_EINVAL, "tile (%d, %d, %d x %d) of a %dx%d frame: %s", tile->x0, tile->y0, tile->w, tile->h, w, h, why);
    return WZ_OK;
}
static hipError_t skewed_copy(const uint8_t* frame, uint64_t bytes, uint8_t** base, const uint8_t** at) {
    hipError_t err = hipMalloc((void**)base, bytes + 16);
    if (err != hipSuccess) return err;
    *at = *base + (reinterpret_cast<uintptr_t>(frame) & 15u);
    return hipMemcpy(const_cast<uint8_t*>(*at), frame, bytes, hipMemcpyHostToDevice);
}

// one tile of one host frame through wz_k_crop_tiles
extern "C" int wz_stage_crop_tile(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, uint8_t* out) {
    if (!e || !frame || !tile || !out) return wz_set_error(WZ_EINVAL, "wz_stage_crop_tile: null argument");
    WZCHK(one_tile_check(w, h, fmt, tile));
    const uint64_t bytes = wz_frame_bytes(w, h, fmt), tbytes = wz_frame_bytes(tile->w, tile->h, fmt);
    if (bytes >> 31) return wz_set_error(WZ_ELIMIT, "frame too large");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    DevBlock<uint8_t> d_src, d_dst;
    const uint8_t* src = nullptr;
    hipError_t err = skewed_copy(frame, bytes, &d_src.p, &src);
    if (err == hipSuccess) err = d_dst.alloc(tbytes);
    if (err == hipSuccess) {
        std::vector<WzCropPlane> planes;
        tile_planes(src, w, h, fmt, *tile, d_dst, planes);
        wz_launch_crop_tiles(planes.data(), (int)planes.size(), e->stream);
        err = hipStreamSynchronize(e->stream);
    }
    if (err == hipSuccess) err = hipMemcpy(out, d_dst, tbytes, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_stage_crop_tile: %s", hipGetErrorString(err));
    return WZ_OK;
}

// wz_k_merge_tiles (+ the camera's filter) on caller-provided tile rows of one w x h frame
extern "C" int wz_stage_merge_tiles(wz_engine_t* e, int w, int h, int cam, int n_tiles, const wz_tile_t* tiles, const wz_detection_t* tile_rows,
                                    double iou_thr, double ios_thr, wz_detection_t* rows, uint8_t* pass) {
    if (!e || !tiles || !tile_rows || !rows || !pass || w < 1 || h < 1) return wz_set_error(WZ_EINVAL, "wz_stage_merge_tiles: bad argument");
    if (n_tiles < 1 || n_tiles > WZ_MAX_TILES) return wz_set_error(WZ_ELIMIT, "%d tiles, a frame takes 1 to %d", n_tiles, WZ_MAX_TILES);
    if (cam >= WZ_MAX_CAMS) return wz_set_error(WZ_ELIMIT, "camera id %d >= %d", cam, WZ_MAX_CAMS);
    if (cam >= 0 && e->h_cams[cam].enabled && (e->h_cams[cam].width != w || e->h_cams[cam].height != h))
        return wz_set_error(WZ_EINVAL, "the frame is %dx%d but camera %d filter was set for %dx%d", w, h, cam, e->h_cams[cam].width, e->h_cams[cam].height);
    for (int t = 0; t < n_tiles; ++t)
        if (tiles[t].w < 1 || tiles[t].h < 1 || tiles[t].x0 < 0 || tiles[t].y0 < 0 || (int64_t)tiles[t].x0 + tiles[t].w > w || (int64_t)tiles[t].y0 + tiles[t].h > h)
            return wz_set_error(WZ_EINVAL, "tile %d (%d, %d, %d x %d) is no rectangle of a %dx%d frame", t, tiles[t].x0, tiles[t].y0, tiles[t].w, tiles[t].h, w, h);
    if (!(iou_thr >= 0.0) || !(ios_thr >= 0.0)) return wz_set_error(WZ_EINVAL, "wz_stage_merge_tiles: the merge thresholds must be numbers >= 0");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t nr = (size_t)n_tiles * WZ_MAX_DETECTIONS;
    struct Parts { wz_detection_t* in; WzMergeFrame* frame; int32_t* org; WzMergeCand* cand; wz_detection_t* rows; uint8_t* pass; size_t bytes; };
    auto carve = [&](const void* base) {   // one device block: the tiles' rows, the frame, its origins, the scratch, the merged rows, their pass bytes
        Carve c(base);
        Parts p = {c.take<wz_detection_t>(nr), c.take<WzMergeFrame>(1), c.take<int32_t>(2 * (size_t)n_tiles), c.take<WzMergeCand>(nr),
                   c.take<wz_detection_t>(WZ_MAX_DETECTIONS), c.take<uint8_t>(WZ_MAX_DETECTIONS), 0};
        p.bytes = c.bytes();
        return p;
    };
    DevBlock<uint8_t> d;
    HIPCHK(d.alloc(carve(nullptr).bytes));
    const Parts p = carve(d);
    const WzMergeFrame fr = {0, n_tiles, cam < 0 ? -1 : cam, 0};
    std::vector<int32_t> org(2 * (size_t)n_tiles);
    for (int t = 0; t < n_tiles; ++t) org[2 * t] = tiles[t].x0, org[2 * t + 1] = tiles[t].y0;
    hipError_t err = hipMemcpy(p.in, tile_rows, sizeof(wz_detection_t) * nr, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(p.frame, &fr, sizeof(fr), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(p.org, org.data(), org.size() * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        wz_launch_merge_tiles(p.frame, p.org, p.in, p.cand, 1, n_tiles, iou_thr, ios_thr, p.rows, p.pass, e->stream);
        if (cam >= 0 && e->h_cams[cam].enabled) wz_launch_filter_rows(e->d_cams, cam, p.rows, p.pass, e->stream);
        err = hipStreamSynchronize(e->stream);
    }
    if (err == hipSuccess) err = hipMemcpy(rows, p.rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(pass, p.pass, WZ_MAX_DETECTIONS, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_stage_merge_tiles: %s", hipGetErrorString(err));
    return WZ_OK;
}

// wz_k_tile_activity on one rectangle of one host frame; with_mask: wz_k_tile_activity<true>, the tile's cells_ignored (null: the tile has no
// mask) as its bits
static int stage_tile_activity(wz_engine_t* e, const char* who, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, const uint16_t* ref,
                               int pixel_thr, bool with_mask, const uint8_t* cells_ignored, uint16_t* sums_out, int32_t* changed_out) {
    if (!e || !frame || !tile || !sums_out || !changed_out) return wz_set_error(WZ_EINVAL, "%s: null argument", who);
    WZCHK(one_tile_check(w, h, fmt, tile));
    const uint64_t bytes = wz_frame_bytes(w, h, fmt);
    if (pixel_thr < 0 || pixel_thr > 255) return wz_set_error(WZ_EINVAL, "pixel_thr %d, expected 0 .. 255", pixel_thr);
    if (bytes >> 31) return wz_set_error(WZ_ELIMIT, "frame too large");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t cells = gate_cells_of(tile->w, tile->h);
    struct Parts { uint16_t *now, *ref; WzGateTile* tile; int32_t* cnt; unsigned long long* ign; size_t bytes; };
    auto carve = [&](const void* base) {   // one device block: new grid, reference grid, the tile's descriptor, the two counters and the count, the mask bits
        Carve c(base);
        Parts p = {c.take<uint16_t>(cells, 16), c.take<uint16_t>(cells, 16), c.take<WzGateTile>(1, 16), c.take<int32_t>(4),
                   c.take<unsigned long long>(ignore_words_of(cells), 16), 0};
        p.bytes = c.bytes();
        return p;
    };
    const size_t all = carve(nullptr).bytes;
    DevBlock<uint8_t> d_src, d;
    const uint8_t* src = nullptr;
    hipError_t err = skewed_copy(frame, bytes, &d_src.p, &src);
    if (err == hipSuccess) err = d.alloc(all);
    if (err == hipSuccess) err = hipMemset(d, 0, all);
    const Parts p = carve(d);
    if (err == hipSuccess && ref) err = hipMemcpy(p.ref, ref, cells * 2, hipMemcpyHostToDevice);
    if (err == hipSuccess && cells_ignored) {
        std::vector<unsigned long long> words(ignore_words_of(cells));
        pack_cell_bits(cells_ignored, cells, words.data());
        err = hipMemcpy(p.ign, words.data(), words.size() * 8, hipMemcpyHostToDevice);
    }
    if (err == hipSuccess) {
        WzGateTile g;
        gate_tile(src, w, fmt, *tile, g);
        if (cells_ignored) g.ignore = reinterpret_cast<const uint32_t*>(p.ign);
        g.ref = ref ? p.ref : nullptr;
        g.now = p.now;
        g.thr = pixel_thr;
        err = hipMemcpy(p.tile, &g, sizeof(g), hipMemcpyHostToDevice);
        if (err == hipSuccess) {
            wz_launch_tile_activity(p.tile, 1, g.crows, g.cols, p.cnt, p.cnt + 2, e->stream, with_mask);
            err = hipStreamSynchronize(e->stream);
        }
    }
    if (err == hipSuccess) err = hipMemcpy(sums_out, p.now, cells * 2, hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(changed_out, p.cnt + 2, 4, hipMemcpyDeviceToHost);
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "%s: %s", who, hipGetErrorString(err));
    return WZ_OK;
}
extern "C" int wz_stage_tile_activity(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, const uint16_t* ref,
                                      int pixel_thr, uint16_t* sums_out, int32_t* changed_out) {
    return stage_tile_activity(e, "wz_stage_tile_activity", frame, w, h, fmt, tile, ref, pixel_thr, false, nullptr, sums_out, changed_out);
}
// ... and as a launch with a masked tile runs it
extern "C" int wz_stage_tile_activity_ignore(wz_engine_t* e, const uint8_t* frame, int w, int h, int fmt, const wz_tile_t* tile, const uint16_t* ref,
                                             int pixel_thr, const uint8_t* cells_ignored, uint16_t* sums_out, int32_t* changed_out) {
    return stage_tile_activity(e, "wz_stage_tile_activity_ignore", frame, w, h, fmt, tile, ref, pixel_thr, true, cells_ignored, sums_out, changed_out);
}

extern "C" int wz_debug_bound_source(wz_engine_t* e, int slot, int32_t* in_place) {
    if (!e || !in_place || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_debug_bound_source: bad argument");
    const Lane& L = e->lanes[slot];
    if (L.bound_src.empty()) return wz_set_error(WZ_EINVAL, "wz_debug_bound_source: lane %d has seen no bound batch", slot);
    memcpy(in_place, L.bound_src.data(), sizeof(int32_t) * L.bound_src.size());
    return WZ_OK;
}

// The mean HIP-event time of `reps` brackets around launch() on stream s, in milliseconds, after three unmeasured ones
template <class F>
static int bracket_ms(hipStream_t s, int reps, F launch, float* mean) {
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    double sum = 0.0;
    for (int r = 0; r < reps + 3; ++r) {
        HIPCHK(hipEventRecord(a, s));
        launch();
        HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        if (r >= 3) sum += ms;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *mean = (float)(sum / reps);
    return WZ_OK;
}

// HIP-event time of the crop launch alone and of the merge launch alone (no filter launch), on lane 0 behind one whole tiled call of the
// same arguments (so that the merge reads real tile rows): the mean of `reps` brackets each, in milliseconds; empty_ms: the same bracket around nothing
extern "C" int wz_profile_tiled(wz_engine_t* e, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt,
                                const int* n_tiles, const wz_tile_t* const* tiles, double iou_thr, double ios_thr, int reps,
                                float* crop_ms, float* merge_ms, float* empty_ms) {
    if (reps < 1 || !crop_ms || !merge_ms || !empty_ms) return wz_set_error(WZ_EINVAL, "wz_profile_tiled: bad argument");
    WZCHK(wz_submit_tiled_device(e, 0, n, d_frames, w, h, fmt, nullptr, n_tiles, tiles, iou_thr, ios_thr));
    WZCHK(wz_wait(e, 0));
    Lane& L = e->lanes[0];
    TileCall c = {n, d_frames, w, h, fmt, nullptr, n_tiles, tiles, iou_thr, ios_thr, 0};
    for (int i = 0; i < n; ++i) c.total += n_tiles[i];
    TilePlan y;
    tile_plan(e, L, c, nullptr, y);
    const TileLane& T = L.tile;
    WZCHK(bracket_ms(L.stream, reps, [&] { wz_launch_crop_tiles(y.planes.data(), (int)y.planes.size(), L.stream); }, crop_ms));
    WZCHK(bracket_ms(L.stream, reps, [&] { wz_launch_merge_tiles(T.meta.m.frames, T.meta.m.origins, L.hrows.d, T.d_tcand, n, y.most, iou_thr, ios_thr, T.trows.d, T.tpass.d, L.stream); },
                     merge_ms));
    return bracket_ms(L.stream, reps, [] {}, empty_ms);   // (two event records with nothing between them: the bracket's own cost)
}

// HIP-event time of the activity launch alone and of the commit launch alone, exactly as one gated call of these arguments on lane 0 issued
// them (their descriptors are still in the lane's block; both launches leave what they wrote the first time): the mean of `reps` brackets
extern "C" int wz_profile_gated(wz_engine_t* e, int n, const uint8_t* const* d_frames, const int* w, const int* h, const int* fmt, const int* cam,
                                double iou_thr, double ios_thr, int reps, float* activity_ms, float* commit_ms, float* empty_ms) {
    if (reps < 1 || !activity_ms || !commit_ms || !empty_ms) return wz_set_error(WZ_EINVAL, "wz_profile_gated: bad argument");
    WZCHK(wz_submit_gated_device(e, 0, n, d_frames, w, h, fmt, cam, iou_thr, ios_thr));
    WZCHK(wz_wait(e, 0));
    Lane& L = e->lanes[0];
    const GateLane& G = L.gate;
    WZCHK(bracket_ms(L.stream, reps, [&] { wz_launch_tile_activity(G.meta.m.tiles, G.g_tiles, G.g_crows, G.g_cols, G.d_gcount, G.meta.m.activity, L.stream, G.g_masked); },
                     activity_ms));
    WZCHK(bracket_ms(L.stream, reps, [&] { wz_launch_gate_commit(G.meta.m.commits, G.g_tiles, L.hrows.d, G.d_grows, L.stream); }, commit_ms));
    return bracket_ms(L.stream, reps, [] {}, empty_ms);
}

// Two caller-provided grids of a w x h frame, the region kernel's scratch, descriptor and output, and a whole-frame tile of the activity
// kernel with its two counters and its count (wz_profile_motion), in one device block
struct MotionStage {
    DevBlock<uint8_t> d;
    uint16_t *now = nullptr, *ref = nullptr;
    uint32_t* scratch = nullptr;
    WzMotionCam* cam = nullptr;
    WzMotionOut* out = nullptr;
    WzGateTile* tile = nullptr;
    int32_t* cnt = nullptr;
    int cells = 0;
    // with_hold (the hold's entry points): + two age grids, and the 100 rows and pass bytes of the stamp kernel
    bool with_hold = false;
    uint8_t *age_in = nullptr, *age_out = nullptr, *pass = nullptr;
    wz_detection_t* rows = nullptr;
    // with_mask (the ignore mask's entry points): + the grid's cell bits
    bool with_mask = false;
    unsigned long long* ignore = nullptr;
    size_t carve(const void* base) {
        Carve c(base);
        now = c.take<uint16_t>(cells, 16); ref = c.take<uint16_t>(cells, 16); scratch = c.take<uint32_t>(cells, 16);
        cam = c.take<WzMotionCam>(1, 16); out = c.take<WzMotionOut>(1); tile = c.take<WzGateTile>(1); cnt = c.take<int32_t>(4);
        if (with_hold) {
            age_in = c.take<uint8_t>(cells, 16); age_out = c.take<uint8_t>(cells, 16);
            rows = c.take<wz_detection_t>(WZ_MAX_DETECTIONS, 16); pass = c.take<uint8_t>(WZ_MAX_DETECTIONS, 16);
        }
        if (with_mask) ignore = c.take<unsigned long long>(ignore_words_of((size_t)cells), 16);
        return c.bytes();
    }
};
static int motion_stage(wz_engine* e, const char* who, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* p, MotionStage& s,
                        const uint8_t* age = nullptr, int hold = 0, int object_hold = 0, const uint8_t* cells_ignored = nullptr) {
    if (!e || !now || !p) return wz_set_error(WZ_EINVAL, "%s: null argument", who);
    WZCHK(motion_refusal(nullptr, who, w, h, fmt, *p));
    if (hold < 0 || hold > 255 || object_hold < 0 || object_hold > 255) return wz_set_error(WZ_EINVAL, "%s: hold and object_hold must be 0 .. 255", who);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    s.cells = (int)gate_cells_of(w, h);
    const size_t all = s.carve(nullptr);
    HIPCHK(s.d.alloc(all));
    s.carve(s.d);
    WzMotionCam d;
    motion_desc(w, h, fmt, *p, s.now, ref ? s.ref : nullptr, s.scratch, d);
    if (s.with_hold) motion_hold_desc(age ? s.age_in : nullptr, s.age_out, hold, object_hold, d);
    if (s.with_mask && cells_ignored) d.ignore = s.ignore;
    HIPCHK(hipMemset(s.d, 0, all));
    if (s.with_mask && cells_ignored) {
        std::vector<unsigned long long> words(ignore_words_of((size_t)s.cells));
        pack_cell_bits(cells_ignored, (size_t)s.cells, words.data());
        HIPCHK(hipMemcpy(s.ignore, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(s.now, now, (size_t)s.cells * 2, hipMemcpyHostToDevice));
    if (ref) HIPCHK(hipMemcpy(s.ref, ref, (size_t)s.cells * 2, hipMemcpyHostToDevice));
    if (s.with_hold && age) HIPCHK(hipMemcpy(s.age_in, age, (size_t)s.cells, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.cam, &d, sizeof(d), hipMemcpyHostToDevice));
    return WZ_OK;
}

// wz_k_motion_regions alone on two caller-provided grids
extern "C" int wz_stage_motion_regions(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion,
                                       int32_t* n_regions, wz_tile_t* regions, int32_t* cells, int32_t* components) {
    if (!n_regions || !regions || !cells || !components) return wz_set_error(WZ_EINVAL, "wz_stage_motion_regions: null argument");
    MotionStage s;
    WZCHK(motion_stage(e, "wz_stage_motion_regions", now, ref, w, h, fmt, motion, s));
    wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    WzMotionOut o;
    HIPCHK(hipMemcpy(&o, s.out, sizeof(o), hipMemcpyDeviceToHost));
    *n_regions = o.n_regions;
    *components = o.components;
    memcpy(regions, o.regions, sizeof(o.regions));
    memcpy(cells, o.cells, sizeof(o.cells));
    return WZ_OK;
}

// HIP-event time of the region launch alone on these grids, and of the whole-frame activity launch of such a frame (constant bytes) alone
extern "C" int wz_profile_motion(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion, int reps,
                                 float* regions_ms, float* activity_ms, float* empty_ms, int32_t* rounds) {
    if (reps < 1 || !rounds || !regions_ms || !activity_ms || !empty_ms) return wz_set_error(WZ_EINVAL, "wz_profile_motion: bad argument");
    MotionStage s;
    WZCHK(motion_stage(e, "wz_profile_motion", now, ref, w, h, fmt, motion, s));
    WZCHK(bracket_ms(e->stream, reps, [&] { wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream); }, regions_ms));
    WzMotionOut o;
    HIPCHK(hipMemcpy(&o, s.out, sizeof(o), hipMemcpyDeviceToHost));
    *rounds = o.rounds;
    const uint64_t bytes = wz_frame_bytes(w, h, fmt);
    DevBlock<uint8_t> d_frame;
    DevBlock<uint16_t> d_grid;
    hipError_t err = d_frame.alloc(bytes);
    if (err == hipSuccess) err = d_grid.alloc((size_t)s.cells);
    if (err == hipSuccess) err = hipMemset(d_frame, 0x55, bytes);
    int rc = WZ_OK;
    if (err == hipSuccess) {
        const wz_tile_t whole = {0, 0, w, h};
        WzGateTile g;
        gate_tile(d_frame, w, fmt, whole, g);
        g.ref = nullptr;
        g.now = d_grid;
        g.thr = 0;
        err = hipMemcpy(s.tile, &g, sizeof(g), hipMemcpyHostToDevice);   // (the counters and the count behind it are zero)
        if (err == hipSuccess) rc = bracket_ms(e->stream, reps, [&] { wz_launch_tile_activity(s.tile, 1, g.crows, g.cols, s.cnt, s.cnt + 2, e->stream); }, activity_ms);
    }
    if (err != hipSuccess) return wz_set_error(WZ_EHIP, "wz_profile_motion: %s", hipGetErrorString(err));
    WZCHK(rc);
    return bracket_ms(e->stream, reps, [] {}, empty_ms);
}

// ---- motion hold
// wz_k_motion_regions<true> alone on two caller-provided grids and the caller's ages
extern "C" int wz_stage_motion_hold(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                                    const wz_motion_t* motion, int hold, int32_t* n_regions, wz_tile_t* regions, int32_t* cells, int32_t* components,
                                    int32_t* active, int32_t* held, uint8_t* age_out) {
    if (!n_regions || !regions || !cells || !components || !active || !held || !age_out) return wz_set_error(WZ_EINVAL, "wz_stage_motion_hold: null argument");
    MotionStage s;
    s.with_hold = true;
    WZCHK(motion_stage(e, "wz_stage_motion_hold", now, ref, w, h, fmt, motion, s, age_in, hold, 0));
    wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream, true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    WzMotionOut o;
    HIPCHK(hipMemcpy(&o, s.out, sizeof(o), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(age_out, s.age_out, (size_t)s.cells, hipMemcpyDeviceToHost));
    *n_regions = o.n_regions;
    *components = o.components;
    *active = o.active;
    *held = o.held;
    memcpy(regions, o.regions, sizeof(o.regions));
    memcpy(cells, o.cells, sizeof(o.cells));
    return WZ_OK;
}

// The ages, rows and pass bytes of one w x h frame in a MotionStage, and the stamp kernel's camera: what wz_k_motion_stamp reads
static int stamp_stage(wz_engine* e, const char* who, const uint8_t* age, const wz_detection_t* rows, const uint8_t* pass, int w, int h, int object_hold,
                       MotionStage& s) {
    if (!e || !age || !rows || !pass) return wz_set_error(WZ_EINVAL, "%s: null argument", who);
    if (w < 1 || h < 1 || object_hold < 0 || object_hold > 255) return wz_set_error(WZ_EINVAL, "%s: a frame of %dx%d, object_hold %d (0 .. 255)", who, w, h, object_hold);
    if (gate_cells_of(w, h) > (size_t)WZ_MOTION_MAX_CELLS)
        return wz_set_error(WZ_ELIMIT, "%s: a %dx%d frame has %zu cells, a motion camera takes at most %d", who, w, h, gate_cells_of(w, h), WZ_MOTION_MAX_CELLS);
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    s.with_hold = true;
    s.cells = (int)gate_cells_of(w, h);
    const size_t all = s.carve(nullptr);
    HIPCHK(s.d.alloc(all));
    s.carve(s.d);
    WzMotionCam d = {};
    d.W = w; d.H = h;
    d.gw = cells_of(w);
    d.gh = cells_of(h);
    motion_hold_desc(nullptr, s.age_out, 0, object_hold, d);
    HIPCHK(hipMemset(s.d, 0, all));
    HIPCHK(hipMemcpy(s.age_out, age, (size_t)s.cells, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.rows, rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.pass, pass, WZ_MAX_DETECTIONS, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.cam, &d, sizeof(d), hipMemcpyHostToDevice));
    return WZ_OK;
}

// wz_k_motion_stamp alone on caller-provided ages, rows and pass bytes
extern "C" int wz_stage_motion_stamp(wz_engine_t* e, const uint8_t* age_in, const wz_detection_t* rows, const uint8_t* pass, int w, int h, int object_hold,
                                     uint8_t* age_out) {
    if (!age_out) return wz_set_error(WZ_EINVAL, "wz_stage_motion_stamp: null argument");
    MotionStage s;
    WZCHK(stamp_stage(e, "wz_stage_motion_stamp", age_in, rows, pass, w, h, object_hold, s));
    wz_launch_motion_stamp(s.cam, 1, s.rows, s.pass, e->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(age_out, s.age_out, (size_t)s.cells, hipMemcpyDeviceToHost));
    return WZ_OK;
}

extern "C" int wz_debug_motion_age(wz_engine_t* e, int cam, uint8_t* out) {
    if (!e || !out) return wz_set_error(WZ_EINVAL, "wz_debug_motion_age: null argument");
    const auto it = e->motion_cams.find(cam);
    if (it == e->motion_cams.end() || !it->second.d_age[0]) return wz_set_error(WZ_EINVAL, "camera %d has no motion hold (wz_set_camera_motion_hold first)", cam);
    const MotionCam& m = it->second;
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    const size_t cells = (size_t)m.gw * m.gh;
    if (!m.has_age) memset(out, 0, cells);
    else HIPCHK(hipMemcpy(out, m.d_age[m.cur], cells, hipMemcpyDeviceToHost));
    return WZ_OK;
}

// HIP-event time of the region launch alone with these ages, and of the stamp launch alone on the ages it left (the stamp raises the same
// cells to the same value every time: every repetition reads and writes what the first did, except that the first finds them lower)
extern "C" int wz_profile_motion_hold(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                                      const wz_motion_t* motion, int hold, const wz_detection_t* rows, const uint8_t* pass, int object_hold, int reps,
                                      float* regions_ms, float* stamp_ms, float* empty_ms) {
    if (reps < 1 || !rows || !pass || !regions_ms || !stamp_ms || !empty_ms) return wz_set_error(WZ_EINVAL, "wz_profile_motion_hold: bad argument");
    MotionStage s;
    s.with_hold = true;
    WZCHK(motion_stage(e, "wz_profile_motion_hold", now, ref, w, h, fmt, motion, s, age_in, hold, object_hold));
    HIPCHK(hipMemcpy(s.rows, rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.pass, pass, WZ_MAX_DETECTIONS, hipMemcpyHostToDevice));
    WZCHK(bracket_ms(e->stream, reps, [&] { wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream, true); }, regions_ms));
    WZCHK(bracket_ms(e->stream, reps, [&] { wz_launch_motion_stamp(s.cam, 1, s.rows, s.pass, e->stream); }, stamp_ms));
    return bracket_ms(e->stream, reps, [] {}, empty_ms);
}

// ---- ignore masks
// wz_k_motion_regions<.., true> alone on two caller-provided grids, the caller's ages and the caller's cell mask.  age_out null: as a camera
// without a hold runs it (<false, true>); cells_ignored null: as a camera without a mask runs inside a launch that has one
extern "C" int wz_stage_motion_ignore(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, const uint8_t* age_in, int w, int h, int fmt,
                                      const wz_motion_t* motion, int hold, const uint8_t* cells_ignored, int32_t* n_regions, wz_tile_t* regions,
                                      int32_t* cells, int32_t* components, int32_t* active, int32_t* held, int32_t* ignored, uint8_t* age_out) {
    if (!n_regions || !regions || !cells || !components || !active || !held || !ignored) return wz_set_error(WZ_EINVAL, "wz_stage_motion_ignore: null argument");
    if (!age_out && (age_in || hold)) return wz_set_error(WZ_EINVAL, "wz_stage_motion_ignore: ages or a hold but no age_out: without age_out the camera has no hold");
    MotionStage s;
    s.with_hold = age_out != nullptr;
    s.with_mask = true;
    WZCHK(motion_stage(e, "wz_stage_motion_ignore", now, ref, w, h, fmt, motion, s, age_in, hold, 0, cells_ignored));
    wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream, s.with_hold, true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    WzMotionOut o;
    HIPCHK(hipMemcpy(&o, s.out, sizeof(o), hipMemcpyDeviceToHost));
    if (age_out) HIPCHK(hipMemcpy(age_out, s.age_out, (size_t)s.cells, hipMemcpyDeviceToHost));
    *n_regions = o.n_regions;
    *components = o.components;
    *active = o.active;
    *held = o.held;
    *ignored = o.ignored;
    memcpy(regions, o.regions, sizeof(o.regions));
    memcpy(cells, o.cells, sizeof(o.cells));
    return WZ_OK;
}

// HIP-event time of the region launch alone on these grids with this cell mask (a camera without a hold)
extern "C" int wz_profile_motion_ignore(wz_engine_t* e, const uint16_t* now, const uint16_t* ref, int w, int h, int fmt, const wz_motion_t* motion,
                                        const uint8_t* cells_ignored, int reps, float* regions_ms, float* empty_ms) {
    if (reps < 1 || !cells_ignored || !regions_ms || !empty_ms) return wz_set_error(WZ_EINVAL, "wz_profile_motion_ignore: bad argument");
    MotionStage s;
    s.with_mask = true;
    WZCHK(motion_stage(e, "wz_profile_motion_ignore", now, ref, w, h, fmt, motion, s, nullptr, 0, 0, cells_ignored));
    WZCHK(bracket_ms(e->stream, reps, [&] { wz_launch_motion_regions(s.cam, 1, s.cells, s.out, e->stream, false, true); }, regions_ms));
    return bracket_ms(e->stream, reps, [] {}, empty_ms);
}
#endif   // WZ_DEV_BUILD

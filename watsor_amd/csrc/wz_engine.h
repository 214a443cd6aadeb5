// Internal to the runtime: struct wz_engine, and what its three files take from each other -- wz_engine.hip (lifecycle, submits,
// filters, the batch around the network), wz_network.hip (what a batch launches for the engine's ops: enqueue_network and its
// load-time twins) and wz_tiles.hip (tiled, gated and tiled frame-table detection).  Nothing here is part of the C ABI: these
// functions keep their C++ names.
//
// Ownership: every block of device or page-locked memory is a DevBlock / MappedBlock member of what uses it -- the engine, a lane, a
// camera, a lane's tile / gate / motion share -- and frees itself with it; what several parts share on purpose is one block handed out
// with Carve.  A lane's captured graphs are GraphForm records, which destroy their HIP objects.  State is built aside and moved in.
// wz_destroy lists nothing: it synchronises, destroys the events and the streams, and deletes the engine.
#pragma once
#include <chrono>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "wz_common.h"

// leave the calling function with the failure of a HIP call as wz_last_error ...
#define HIPCHK(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return wz_set_error(WZ_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                                                  __FILE__, __LINE__);                                     \
    } while (0)
// ... and of a step that answers in the library's own codes (wz_last_error is already set)
#define WZCHK(expr)                     \
    do {                                \
        const int _rc = (expr);         \
        if (_rc != WZ_OK) return _rc;   \
    } while (0)

struct wz_engine;

// Scratch with one owner: a hipMalloc block of T[n], and a page-locked block the device sees too (host pointer and device view).  Move-only:
// a lane's or a camera's scratch is built aside and moved in, all or nothing; what is left behind, or never moved, frees itself.
template <class T>
struct DevBlock {
    T* p = nullptr;
    DevBlock() = default;
    DevBlock(DevBlock&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBlock& operator=(DevBlock&& o) noexcept { std::swap(p, o.p); return *this; }   // (o takes the old block with it)
    ~DevBlock() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, sizeof(T) * n); }
    operator T*() const { return p; }
};
template <class T>
struct MappedBlock {
    T *h = nullptr, *d = nullptr;
    MappedBlock() = default;
    MappedBlock(MappedBlock&& o) noexcept : h(o.h), d(o.d) { o.h = o.d = nullptr; }
    MappedBlock& operator=(MappedBlock&& o) noexcept { std::swap(h, o.h); std::swap(d, o.d); return *this; }
    ~MappedBlock() { if (h) (void)hipHostFree(h); }
    // mapped (hipHostMallocMapped): the device must see the block.  Not mapped (hipHostMallocDefault): d is its device view where the
    // platform gives one, else null
    hipError_t alloc(size_t n, bool mapped = true) {
        hipError_t err = hipHostMalloc((void**)&h, sizeof(T) * n, mapped ? hipHostMallocMapped : hipHostMallocDefault);
        if (err != hipSuccess) return err;
        err = hipHostGetDevicePointer((void**)&d, h, 0);
        if (err == hipSuccess || mapped) return err;
        (void)hipGetLastError();
        d = nullptr;
        return hipSuccess;
    }
};
// A block handed out in typed parts, in order, each at a boundary of `align` bytes (8: every part here holds pointers or 32-bit words).
// On a null base it only measures -- bytes() is what to allocate --; on the host and on the device pointer of one block it gives the two
// views of one layout.
struct Carve {
    uintptr_t base;
    size_t off = 0;
    explicit Carve(const void* b) : base(reinterpret_cast<uintptr_t>(b)) {}
    template <class T>
    T* take(size_t n, size_t align = 8) {
        off = (off + align - 1) & ~(align - 1);
        T* part = reinterpret_cast<T*>(base + off);
        off += sizeof(T) * n;
        return part;
    }
    size_t bytes() const { return (off + 7) & ~(size_t)7; }
};
// A lane's page-locked block of max_batch descriptors of each part of a view V (V::carve), as the host (h) and as the device (m) sees it
template <class V>
struct MetaBlock {
    MappedBlock<uint8_t> block;
    V h = {}, m = {};
    hipError_t alloc(size_t nb) {
        const hipError_t err = block.alloc(h.carve(nullptr, nb));
        if (err == hipSuccess) { h.carve(block.h, nb); m.carve(block.d, nb); }
        return err;
    }
};

// Everything a lane knows about one graph key (batch size | row-staged resize kernel << 16).  Owns its HIP objects; move-only.
struct GraphForm {
    hipGraphExec_t exec = nullptr;       // the instantiated graph; null: nothing was captured under the key (yet)
    hipGraph_t src = nullptr;            // the captured graph itself, kept where one of its node handles is ...
    hipGraphNode_t pre_node = nullptr;   // ... the resize kernel's node: its arguments carry the frame descriptors and are rewritten
                                         // before every replay, if it takes them by value
    int nodes = 0;                       // nodes of the captured graph (kernels + the descriptor copy)
    int post_mode = 0;                   // development library: decode_fused | cands_listed << 1 of the batch enqueued or captured under the key
    std::vector<WzLaunchNote> notes;     // stamps build: what was launched, in order (grid, block, LDS, kernel)
    bool noted = false;                  // ... taken: at capture, or at the key's first kernel-by-kernel enqueue
    WzPreArgs args;                      // storage behind the node's kernelParams
    GraphForm() = default;
    GraphForm(GraphForm&& o) noexcept { *this = std::move(o); }
    GraphForm& operator=(GraphForm&& o) noexcept {   // (o takes the old objects with it)
        std::swap(exec, o.exec); std::swap(src, o.src); std::swap(pre_node, o.pre_node); std::swap(nodes, o.nodes);
        std::swap(post_mode, o.post_mode); notes.swap(o.notes); std::swap(noted, o.noted);
        return *this;
    }
    ~GraphForm() {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (src) (void)hipGraphDestroy(src);
    }
};

// tiled detection (wz_submit_tiled_device / wz_detect_tiled): a lane's share, allocated the first time the lane sees a tiled call
struct TileMeta {
    WzMergeFrame* frames;                // the merge launch's frames [max_batch]
    int32_t* origins;                    // the tiles' origins (x0, y0) [max_batch][2]
    size_t carve(const void* base, size_t nb) {
        Carve c(base);
        frames = c.take<WzMergeFrame>(nb); origins = c.take<int32_t>(2 * nb);
        return c.bytes();
    }
};
struct TileLane {
    DevBlock<uint8_t> d_tiles;           // tile staging [max_batch][frame_stride]: the crop launch's output, the batch's frames
    DevBlock<WzMergeCand> d_tcand;       // the merge kernel's scratch [max_batch][100]
    MappedBlock<wz_detection_t> trows;   // the merged rows [max_batch][100] ...
    MappedBlock<uint8_t> tpass;          // ... and their pass bytes, written by the merge launch (and the filter launches behind it)
    MetaBlock<TileMeta> meta;
    int tiled = 0;                       // frames of the tiled batch in flight (its rows are in trows.h); 0: the batch is not tiled
    int alloc(wz_engine* e);             // (wz_tiles.hip) lazy; all or nothing
    void release() { *this = TileLane(); }
};
// gated tiled detection (wz_submit_gated_device / wz_detect_gated): allocated the first time the lane sees a gated call
struct GateMeta {
    WzGateTile* tiles;                   // the activity launch's tiles [max_batch]
    WzGateCommit* commits;               // the commit launch's [max_batch]
    int32_t* activity;                   // the activity counts [max_batch]
    size_t carve(const void* base, size_t nb) {
        Carve c(base);
        tiles = c.take<WzGateTile>(nb); commits = c.take<WzGateCommit>(nb); activity = c.take<int32_t>(nb);
        return c.bytes();
    }
};
struct GateLane {
    DevBlock<uint16_t> d_gnow;           // the activity launch's new grids [max_batch][gate_cells]
    DevBlock<wz_detection_t> d_grows;    // fresh or cached rows of every tile of the call, in tile order [max_batch][100]: what the merge reads
    DevBlock<int32_t> d_gcount;          // the activity kernel's counters [max_batch][2]
    MetaBlock<GateMeta> meta;
    std::vector<uint64_t> g_ran;         // the last gated call accepted on this lane (wz_gate_stats): per frame, bit t = tile t ran ...
    std::vector<int32_t> g_act;          // ... and every tile's activity, in tile order
    int g_tiles = 0, g_crows = 0, g_cols = 0;   // that call's launches: tiles, the most cell rows / columns of a tile
    bool g_masked = false;                      // ... and whether one of its cameras had an ignore mask
    int alloc(wz_engine* e);
    void release() { *this = GateLane(); }
};
// motion regions (wz_submit_motion_device / wz_detect_motion): allocated the first time the lane sees a motion call
struct MotionMeta {
    WzGateTile* tiles;                   // the activity launch's whole-frame tiles [max_batch]
    WzMotionCam* cams;                   // the region launch's cameras [max_batch]
    WzMotionOut* outs;                   // what it found [max_batch]
    int32_t* activity;                   // the activity counts [max_batch] (unused)
    size_t carve(const void* base, size_t nb) {
        Carve c(base);
        tiles = c.take<WzGateTile>(nb); cams = c.take<WzMotionCam>(nb); outs = c.take<WzMotionOut>(nb); activity = c.take<int32_t>(nb);
        return c.bytes();
    }
};
struct MotionLane {
    DevBlock<uint32_t> d_mscratch;       // the region kernel's scratch [max_batch][cam_words]
    DevBlock<int32_t> d_mcount;          // the activity kernel's counters [max_batch][2]
    MetaBlock<MotionMeta> meta;
    size_t cam_words = 0;
    std::vector<int32_t> s_ntiles, s_cells, s_comps;   // the last motion call accepted on this lane (wz_motion_stats): per frame its tiles,
    std::vector<wz_tile_t> s_tiles;                    // [n][1 + WZ_MOTION_MAX_REGIONS], its regions' n [n][WZ_MOTION_MAX_REGIONS], its components
    std::vector<int32_t> s_active, s_held;             // ... and (wz_motion_hold_stats) its active cells and those of them that did not change
    std::vector<int32_t> s_ignored;                    // ... and (wz_motion_ignore_stats) the changed cells its camera's ignore mask removed
    int alloc(wz_engine* e);             // (wz_tiles.hip) lazy; all or nothing
    void release() { *this = MotionLane(); }
};

struct wz_engine {
    int device = 0;
    hipStream_t stream = nullptr;            // = lanes[0].stream (stage-level entry points, filters)
    std::string name;
    std::vector<uint8_t> blob;
    WzBlobHeader hdr;
    const WzTensorDesc* tensors = nullptr;
    const WzOpDesc* ops = nullptr;
    int max_batch = 0, max_w = 0, max_h = 0;
    bool no_reuse = false, use_graph = true, use_splitk = true;
    bool graph_adaptive = false;   // use_graph && WZ_GRAPH unset: a batch that finds every other lane idle is launched kernel by kernel (wz_create)
    bool fuse_decode = true;   // WZ_FUSE_DECODE=0: keep wz_k_decode as its own launch
    bool defer_heads = true;   // the SSD heads' split-K reductions run as one launch after the last head (WZ_DEFER_HEADS=0: one each)
    bool conv_wide = true;     // the big SSD heads on the wide tile kernel (k_conv_wide.hip); WZ_CONV_WIDE=0: on wz_k_conv_rs
    int wide_min_m = 1;        // WZ_WIDE_MIN_M=n: heads with fewer output pixels than this (per batch) stay on wz_k_conv_group
    int wide_T = 0;            // WZ_WIDE_T=n: K steps per slice of that kernel (0: chosen per launch by wz_choose_wide_T)
                                  // 2 (round 5): only the chain behind the 3x3 map -- its last four convolutions, 0.8 MB of weights per frame's workgroup
    bool desc_by_value = true;    // the frame descriptors travel as arguments of the resize kernel (WZ_DESC_ARGS=0: zero-copy / copied)
    bool desc_zero_copy = true;   // the resize kernel reads the frame descriptors from page-locked host memory (WZ_DESC_COPY=1: copied first)
    bool pre_rows = false;        // WZ_PRE_ROWS=1: every batch on the row-staged form of the resize kernel (k_preprocess.hip:
                                  // wz_k_preprocess_rows); default: only batches with a frame that is read in place (the per-pixel form is
                                  // faster out of HBM: 51.5 k against 48.0 k frames/s on the headline workload, profiles/r04_host_read_ab.txt)
    int pre_rows_lds = 0;         // ... and its LDS bytes for the widest frame this engine takes
    int host_read = 2;            // page-locked host frames (WZ_HOST_READ): 0 = staged by one DMA each, 1 = read in place by the resize kernel
                                  // (no copy), 2 (default) = read in place when the resize skips rows (vertical down-scale >= 2: 1080p RGB24
                                  // 8.0 k -> 13.0 k frames/s, NV12 15.6 k -> 18.7 k), staged otherwise (640x480 in place: 26 k against 33 k)
    struct HostRange { const uint8_t* host; uint64_t bytes; const uint8_t* dev; };
    std::vector<HostRange> host_ranges;   // what wz_host_register page-locked, with the address the device sees it at
    int wide_cus = 128;        // CUs the wide head kernel's K slices are sized for when several lanes are in flight (WZ_WIDE_CUS)
    int num_cus = 256;         // compute units of the device (the wide head kernel sizes its K slices for one round over them)

    DevBlock<uint8_t> d_weights;
    DevBlock<half_t> d_zeros;                // 4 KiB of zeros
    DevBlock<unsigned long long> d_mbdbg;    // WZ_MB_DEBUG=1: [n_ops][16] phase timestamps of the fused-block kernels
    std::vector<int> mb_groups;
    DevBlock<float> d_anchors;
    size_t frame_stride = 0;                 // bytes of one frame of a lane's staging area (max_w * max_h * 3, rounded up to 256)
    WzPostConsts pc;
    size_t post_scratch_bytes = 0;
    size_t ws_bytes = 0;       // split-K / channel-group workspace per lane: 32 MiB per frame of max_batch, at least 64 MiB (the heads'
                               // parked partial sums take ~10 MiB per frame, the other ops keep the lower half)

    // A lane is everything one in-flight batch needs: its own stream, activation buffers, head
    // outputs, post-processing scratch, descriptor/result blocks and captured graphs.  Lanes run
    // concurrently on the GPU (a batch-8 layer fills only a fraction of the 256 CUs), slot i of the
    // API is lane i.
    struct Lane {
        hipStream_t stream = nullptr;
        bool owns_stream = false;            // false: the stream belongs to lane (index mod n_streams)
        std::vector<DevBlock<uint8_t>> bufs; // the activation buffers
        std::vector<half_t*> tptr;           // tensor index -> device pointer
        DevBlock<float> d_box_enc, d_logits, d_ws;
        int launch_failed = 0;               // op index + 1 of a block no kernel took at launch time (enqueue_network), else 0
        bool decode_fused = false;           // set by enqueue_network: the grouped head reduce decoded the boxes
        bool cands_listed = false;           // ... and listed the candidates of the NMS kernel's first band
        DevBlock<uint8_t> d_frames;          // staging for host frames of this lane [max_batch][frame_stride]
        WzPostBuffers post;                  // what the kernels take: views of the blocks below (and of d_box_enc, d_logits, the engine's anchors)
        DevBlock<uint32_t> d_post_scratch;   // post.hint, post.hint_logit, post.cbits
        DevBlock<float> d_boxes, d_det_boxes, d_det_scores;
        DevBlock<uint8_t> d_valid;
        DevBlock<int32_t> d_det_classes, d_det_num;
        DevBlock<unsigned long long> d_dbg;
        MappedBlock<WzFrameDesc> desc;       // page-locked, not mapped: desc.d is null where the device does not see it
        // the descriptors in device memory.  WZ_LANE_STAMPS builds (wz_common.h): the lane's launch blocks [WZ_STAMP_SLOTS][WZ_STAMP_WORDS], the
        // resize kernel's block and the descriptors behind it are ONE block, carved (lane_parts)
        DevBlock<uint8_t> d_parts;
        WzFrameDesc* d_desc = nullptr;
        unsigned long long* d_stamps = nullptr;
        unsigned long long* d_stamps_pre = nullptr;
        MappedBlock<wz_detection_t> hrows;   // page-locked, device-mapped: the NMS kernel writes the rows straight into it ...
        MappedBlock<uint8_t> hpass;          // ... and their pass bytes
        MappedBlock<uint32_t> hstatus;       // one word per frame, non-zero = the frame's rows may be short (wz_k_nms)
        MappedBlock<unsigned long long> hstamps;   // stamps build: the page-locked pairs the host reads
        std::vector<int32_t> bound_idx;      // frame-table entries of the batch in flight (empty: not a bound batch)
        std::vector<int32_t> bound_src;      // the last tiled, gated or motion bound batch accepted on this lane (development library: the last bound batch of any kind): 1 = frame i was read in place, 0 = staged
        TileLane tile;
        GateLane gate;
        MotionLane motion;
        hipEvent_t done = nullptr;
        int n = 0;
        bool rows = false;                       // the batch being enqueued runs the row-staged resize kernel (a frame of it is read in place)
        int key = 0;                             // graph key of the batch in flight: batch size | rows << 16
        std::map<int, GraphForm> forms;          // graph key -> its record
        int stamp_next = 1;                      // stamps build: launches stamped so far in the batch being enqueued
        bool lone = false;                       // the batch being enqueued goes kernel by kernel because the other lanes are idle (run_batch)
    };
    Lane lanes[WZ_SLOTS];
    int n_lanes = 4;   // default; WZ_LANES overrides (1..WZ_SLOTS)
    int n_streams = 4; // HIP streams the lanes are spread over (WZ_STREAMS); more than 4 run slower on this stack (HISTORY.md part B)

    // the worker's frame table (wz_bind_frames): one entry per Frame of every FrameBuffer, described once instead of once per batch
    struct BoundFrame {
        const uint8_t* host;   // the frame's pixels (host address)
        const uint8_t* dev;    // the same bytes as the device sees them when the frame lies in a wz_host_register range, else nullptr
        int32_t w, h, fmt, cam;
        uint64_t bytes;
        wz_detection_t* rows;  // Header.detections of that frame (host), written by wz_collect_bound
    };
    std::vector<BoundFrame> bound;
    // the tiled description of a table entry (wz_bind_tiles).  Kept beside the table, and EMPTY while no entry has one: the untiled
    // wz_submit_bound looks at nothing but that.
    enum { BOUND_PLAIN = 0, BOUND_TILED = 1, BOUND_GATED = 2, BOUND_MOTION = 3 };
    struct BoundTiles {
        int kind = BOUND_PLAIN;
        std::vector<wz_tile_t> tiles;   // BOUND_TILED: the entry's rectangles (BOUND_GATED: its camera's, looked up at submit; BOUND_MOTION
                                        // (wz_bind_motion): none -- its camera's settings, hold and mask are looked up at submit, the region launch finds the rectangles)
        double iou = 0.0, ios = 0.0;    // the merge thresholds of the three kinds
    };
    std::vector<BoundTiles> bound_tiles;   // [bound.size()] or empty

    std::vector<WzCamFilter> h_cams;
    DevBlock<WzCamFilter> d_cams;
    std::vector<DevBlock<int32_t>> cam_sat;   // the summed-area tables of the cameras' zone masks (WzCamFilter::sat points into them)
    DevBlock<wz_detection_t> d_tmp_rows;      // one frame's rows and pass bytes in device memory (wz_filter_rows, wz_stage_rows)
    DevBlock<uint8_t> d_tmp_pass;

    // gated tiled detection: a camera's tile layout and its state in device memory (wz_set_camera_tiles); empty until a camera is set
    struct GateCam {
        int w = 0, h = 0, base = 0;              // the frames this layout was set for: size and base format
        wz_tile_gate_t gate = {0, 1, 0, 0};
        std::vector<wz_tile_t> tiles;
        std::vector<int> cols, crows;            // cells of every tile
        std::vector<size_t> grid_off;            // first cell of every tile's reference grid in d_ref
        DevBlock<uint16_t> d_ref;                // the tiles' reference grids, one after the other
        DevBlock<wz_detection_t> d_rows;         // the tiles' cached rows [tiles][100]
        std::vector<uint8_t> has_ref;            // the tile has a reference (and cached rows)
        std::vector<int> skipped;                // gated calls of this camera in a row that skipped the tile
        int lane = -1;                           // the lane whose gated batch last wrote this state
        // ignore mask (wz_set_camera_ignore): every tile's cell bits, one after the other; null: the camera has none
        DevBlock<uint32_t> d_ignore;
        std::vector<size_t> ignore_off;          // first 32-bit word of every tile's bits in d_ignore
        void release() { *this = GateCam(); }    // frees the device blocks
    };
    std::map<int, GateCam> gate_cams;
    // motion regions: a camera's settings and its two whole-frame grids (wz_set_camera_motion); empty until a camera is set.  The grid the
    // last accepted call wrote is the reference of the next one: the two are swapped by pointer, nothing is copied.
    // A camera with a hold (wz_set_camera_motion_hold) has two age grids beside them, swapped by the same `cur`: the region launch reads
    // d_age[cur] and writes d_age[cur ^ 1], the stamp launch -- still in flight when the call returns -- raises d_age[cur ^ 1].
    struct MotionCam {
        int w = 0, h = 0, base = 0, fmt = 0;     // the frames the settings were made for
        int gw = 0, gh = 0;                      // cells of the whole frame
        wz_motion_t p = {0, 1, 0, 1, 16, 0, 0, 0};
        DevBlock<uint16_t> d_grid[2];
        int cur = 0;                             // d_grid[cur] is the reference, d_grid[cur ^ 1] takes the next call's grid
        bool has_ref = false;
        DevBlock<uint8_t> d_age[2];              // null: the camera has no hold
        bool has_age = false;                    // d_age[cur] holds ages (false: they are all zero, whatever the grid says)
        int hold = 0, object_hold = 0;
        int lane = -1;                           // the lane whose motion call last stamped d_age
        DevBlock<unsigned long long> d_ignore;   // ignore mask (wz_set_camera_ignore): the frame grid's cell bits; null: the camera has none
        void release() { *this = MotionCam(); }  // frees the grids
    };
    std::map<int, MotionCam> motion_cams;

    std::vector<std::string> stage_names;   // stage_slots(op) names per op, between the fixed ones (wz_create)
    // what the op list alone says about op i (network_prepare): the next op is the only reader of its output (the extras pair's
    // structural precondition); its source tensor holds every value twice (its writer has WZ_OPF_DUP_OUT)
    struct OpFacts { uint8_t sole_next, dup_k; };
    std::vector<OpFacts> op_facts;
};
typedef wz_engine::Lane Lane;

static inline int input_tensor_index(const wz_engine* e) { return e->ops[0].src; }
static inline bool tensor_is_pair(const wz_engine* e, int idx) { return (e->tensors[idx].flags & WZ_TENSOR_HP) != 0; }
static inline bool input_is_pair(const wz_engine* e) { return tensor_is_pair(e, input_tensor_index(e)); }

// wz_profile_stages: one event per mark, a stage = the bracket between two marks
struct StageTimer {
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    hipStream_t s = nullptr;
    void mark() {
        if (used == ev.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            ev.push_back(e);
        }
        (void)hipEventRecord(ev[used++], s);
    }
};

// ---- wz_network.hip, for wz_engine.hip ---------------------------------------------------------------------------------------------
int stage_slots(const WzOpDesc& op);   // stage-timer brackets an op owns: 2 (launch, reduce) for a convolution or a fused block, else 1
int op_kernel_check(wz_engine* e, const WzOpDesc& op, const char* path);   // load_blob: a kernel exists for the op's shape, or WZ_EFORMAT
void network_prepare(wz_engine* e);    // wz_create: kernel attributes on the engine's device, op_facts
WzConvArgs conv_args(wz_engine* e, const Lane& L, const WzOpDesc& op, int n);
void head_outputs(wz_engine* e, const Lane& L, const WzOpDesc& op, WzConvArgs& a);
void enqueue_network(wz_engine* e, Lane& L, int n, StageTimer* t, bool with_post = true);
#ifdef WZ_DEV_BUILD
int enqueue_block_at(wz_engine* e, Lane& L, int n, uint32_t op_index, const void* d_in, int launch_frames);   // one fused block, its source tensor at d_in; -1: not a block / no kernel
#endif

// ---- wz_engine.hip, for wz_tiles.hip --------------------------------------------------------------------------------------------
const char* fmt_refusal(int w, int h, int fmt);
int fill_desc(wz_engine* e, int slot, int n, const uint8_t* const* d_rgb, const int* w, const int* h, const int* fmt, const int* cam);
int run_batch(wz_engine* e, int slot, int n);
int stage_frame(wz_engine* e, Lane& L, int i, const uint8_t* host, uint64_t bytes, const uint8_t** where);
int collect_timed(wz_engine* e, int n, wz_detection_t* const* out, uint8_t* const* pass, float* ms, std::chrono::steady_clock::time_point t0);
const uint8_t* device_view(wz_engine* e, const uint8_t* host, uint64_t bytes);
bool read_in_place(const wz_engine* e, int h);
bool rows_fit(const wz_engine* e, int n, const int* w, const int* fmt);
int sync_all(wz_engine* e);
hipError_t lane0_fill(wz_engine* e, void* dst, int value, size_t bytes);
// ---- wz_tiles.hip, for wz_submit_bound: a batch with a tiled, gated or motion entry ---------------------------------------------------------
int submit_bound_tiles(wz_engine* e, int slot, int n, const int32_t* entries);

// Why a call's lane or batch size is refused (wz_last_error is set, the code returned), or WZ_OK: the checks named in `checks`, in this order
enum { BC_SLOT = 1, BC_N = 2 };
static inline int batch_refusal(const wz_engine* e, int slot, int n, unsigned checks = BC_SLOT | BC_N) {
    if ((checks & BC_SLOT) && (slot < 0 || slot >= e->n_lanes)) return wz_set_error(WZ_EINVAL, "slot %d out of range [0,%d)", slot, e->n_lanes);
    if ((checks & BC_N) && (n < 1 || n > e->max_batch)) return wz_set_error(WZ_ELIMIT, "batch %d exceeds max_batch %d", n, e->max_batch);
    return WZ_OK;
}
// Why frame i of a call is refused (wz_last_error is set, the code returned), or WZ_OK: the checks named in `checks`, in this order.
// what: "frame" | "frame-table entry"; p: the frame's pointer, null also when another pointer of the frame is; pf: its format word.
enum { FC_PTR = 1, FC_FMT = 2, FC_LIMIT = 4, FC_CAM_ID = 8, FC_CAM_FILTER = 16 };
static inline int frame_refusal(const wz_engine* e, const char* what, int i, const void* p, int w, int h, int pf, int cam, unsigned checks) {
    if ((checks & FC_PTR) && (!p || w < 1 || h < 1)) return wz_set_error(WZ_EINVAL, "%s %d: bad pointer or size", what, i);
    if ((checks & FC_FMT) && !wz_frame_bytes(w, h, pf))
        return wz_set_error(WZ_EINVAL, "%s %d: pixel format 0x%x at %dx%d: %s", what, i, pf, w, h, fmt_refusal(w, h, pf));
    if ((checks & FC_LIMIT) && (w > e->max_w || h > e->max_h || (size_t)w * h * 3 > e->frame_stride))
        return wz_set_error(WZ_ELIMIT, "%s %d is %dx%d, engine was created for at most %dx%d", what, i, w, h, e->max_w, e->max_h);
    if ((checks & FC_CAM_ID) && cam >= WZ_MAX_CAMS) return wz_set_error(WZ_ELIMIT, "camera id %d >= %d", cam, WZ_MAX_CAMS);
    if ((checks & FC_CAM_FILTER) && cam >= 0 && e->h_cams[cam].enabled && (e->h_cams[cam].width != w || e->h_cams[cam].height != h))
        return wz_set_error(WZ_EINVAL, "%s %d is %dx%d but camera %d filter was set for %dx%d", what, i, w, h, cam, e->h_cams[cam].width,
                            e->h_cams[cam].height);
    return WZ_OK;
}

// A bound batch's table entries as the arrays fill_desc and the tile checks take: one pass over the table, two allocations.
struct BoundBatch {
    std::vector<const uint8_t*> ptr;   // the frames' host addresses; the caller replaces each by where the device finds the frame
    std::vector<int> v;                // w, h, fmt, cam: [4][n]
    int *w, *h, *fmt, *cam;
};
static inline void bound_gather(const wz_engine* e, int n, const int32_t* entries, BoundBatch& b) {
    b.ptr.resize(n);
    b.v.resize(4 * (size_t)n);
    b.w = b.v.data(); b.h = b.w + n; b.fmt = b.h + n; b.cam = b.fmt + n;
    for (int i = 0; i < n; ++i) {
        const wz_engine::BoundFrame& f = e->bound[entries[i]];
        b.ptr[i] = f.host; b.w[i] = f.w; b.h[i] = f.h; b.fmt[i] = f.fmt; b.cam[i] = f.cam;
    }
}
// ... and the lane they go to, drained: its previous batch (and its reads of the staging area) is done
static inline int bound_drain(wz_engine* e, int slot) {
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->lanes[slot].done));
    return WZ_OK;
}

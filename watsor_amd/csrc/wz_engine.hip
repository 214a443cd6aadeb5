// Runtime + C ABI of libwatsor_hip.so (see include/watsor_hip.h for the contract of every entry point).
//
// One engine = one MI355X = a few lanes (wz_engine.h).  A batch is one dependent chain of kernels
// (pre-process -> ~70 conv ops -> post-process -> rows) captured once per (lane, batch size, resize form) into a
// hipGraph and replayed; the frame descriptors travel as the resize kernel's arguments, rewritten in the captured node
// before every replay, results come back through a page-locked row block that the last kernel fills.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>

#include "wz_engine.h"

// Lanes are HIP streams; ROCclr multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and two
// lanes sharing one queue serialise (measured: 4 lanes 23k frames/s on 4 queues, 34k on 8).  The variable is read
// when the HIP runtime initialises, i.e. at the first HIP call, which cannot precede this constructor -- unless the
// process initialised HIP before it loaded this library (wz_hw_queues() still tells what the constructor left).
// The library needs 8 and takes them whatever the host pinned below that (unset, empty, not a number, 1 .. 7: set
// to 8); a host that chose 8 or more keeps its choice -- never raised, never lowered, nothing above 32 is written.
static const char kHwQueuesVar[] = "GPU_MAX_HW_QUEUES";
static const int kHwQueuesNeeded = 8;
static int wz_env_hw_queues() {   // the variable as a number; 0: unset, empty or not a number
    const char* v = getenv(kHwQueuesVar);
    if (!v || !v[0]) return 0;
    char* end = nullptr;
    const long n = strtol(v, &end, 10);
    while (*end == ' ' || *end == '\t') ++end;
    return (*end || n < 1 || n > 1 << 20) ? 0 : (int)n;
}
#ifndef WZ_KEEP_HOST_HW_QUEUES   // (a scratch measurement build leaves the host's value in force: DESIGN.md section 5)
__attribute__((constructor)) static void wz_runtime_defaults() {
    if (wz_env_hw_queues() < kHwQueuesNeeded) setenv(kHwQueuesVar, "8", 1);
}
#endif
extern "C" int wz_hw_queues(void) { return wz_env_hw_queues(); }

thread_local int wz_launch_repeat = 1;
static thread_local char g_err[512] = "";
int wz_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// lane stamps (`make stamps` only): what the batch being enqueued launches is noted where run_batch points the sink
#if WZ_LANE_STAMPS
static thread_local std::vector<WzLaunchNote>* g_launch_sink = nullptr;
void wz_note_launch(const void* func, dim3 grid, dim3 block, size_t lds) {
    if (g_launch_sink) g_launch_sink->push_back({func, {grid.x, grid.y, grid.z}, {block.x, block.y, block.z}, (unsigned)lds});
}
#endif
// bytes of one frame of tensor idx (pair tensors hold two halves per value; the input tensor is fp16 in both engines)
static size_t tensor_frame_bytes(wz_engine* e, int idx) {
    const WzTensorDesc& t = e->tensors[idx];
    const size_t es = idx == input_tensor_index(e) ? 2 : e->hdr.precision / 8;
    return (size_t)t.h * t.w * t.c * es * (tensor_is_pair(e, idx) ? 2 : 1);
}

// ------------------------------------------------------------------------------------------------
// pipeline
// ------------------------------------------------------------------------------------------------
static void enqueue_post(wz_engine* e, Lane& L, bool rows, int n, StageTimer* t, bool decode_done = false, bool listed = false) {
    hipStream_t s = L.stream;
    if (!decode_done) wz_launch_decode(L.post, e->pc, n, s);
    if (t) t->mark();
    // the NMS kernel selects its candidates itself, one workgroup per frame
    // with `rows` the NMS kernel also fills the Detection rows (straight into the lane's pinned, device-mapped host
    // block: no D2H copy node, no separate row kernel); the "post/rows" stage slot stays empty
#if WZ_LANE_STAMPS
    L.post.stamps_n = rows && L.hstamps.d ? L.stamp_next : 0;   // launches stamped in front of the NMS kernel (launch 0 = the resize kernel)
    L.post.stamps_host = rows && L.post.stamps_n ? L.hstamps.d : nullptr;
#endif
    if (rows)
        wz_launch_nms(L.post, e->pc, n, s, L.d_desc, e->d_cams, L.hrows.d, L.hpass.d, listed, L.hstatus.d);
    else
        wz_launch_nms(L.post, e->pc, n, s, nullptr, nullptr, nullptr, nullptr, listed);
    if (t) t->mark();
    if (rows && t) t->mark();
}

// the resize launch of a batch of n on lane L: which kernel, its shape, its last argument (k_preprocess.hip)
static WzPreLaunch pre_launch(const wz_engine* e, const Lane& L, int n) {
    return wz_preprocess_launch(input_is_pair(e), n, (int)e->hdr.input_size, L.rows ? e->pre_rows_lds : 0, e->hdr.resize_mode == 1);
}

// everything between "descriptors are in desc.h" and "rows are in hrows.h"; F: the record of the batch's graph key
// inner > 1 (profiling only): every kernel of the pre-processing and the network is enqueued `inner` times back to back
static void enqueue_batch(wz_engine* e, Lane& L, GraphForm& F, int n, StageTimer* t, int inner = 1) {
    hipStream_t s = L.stream;
    if (t) t->mark();   // "(empty)": two event records with nothing between them = the bracket's own cost
    // the descriptors: read by the resize kernel straight out of the lane's page-locked host block (and left in d_desc for the
    // kernels behind it), or -- WZ_DESC_COPY=1, and where the host block has no device address -- copied in front of it
    // (by value: the descriptors are the resize kernel's arguments -- no copy, no PCIe read; batches of more than WZ_DESC_PACK frames
    // and WZ_DESC_ARGS=0 take one of the older routes)
    const bool by_value = e->desc_by_value && n <= WZ_DESC_PACK;
    const bool zero_copy = !by_value && e->desc_zero_copy && L.desc.d;
    if (!by_value && !zero_copy) (void)hipMemcpyAsync(L.d_desc, L.desc.h, sizeof(WzFrameDesc) * n, hipMemcpyHostToDevice, s);
    if (t) t->mark();
    wz_launch_repeat = inner;
    L.stamp_next = 1;   // (lane stamps: launch 0 is the resize kernel, whose block lies in front of the descriptors it leaves behind)
    wz_launch_preprocess(zero_copy ? L.desc.d : L.d_desc, n, (int)e->hdr.input_size, L.tptr[input_tensor_index(e)], s,
                         input_is_pair(e), (zero_copy || by_value) ? L.d_desc : nullptr, e->hdr.resize_mode == 1,
                         by_value ? L.desc.h : nullptr, L.rows ? e->pre_rows_lds : 0);
    if (t) t->mark();
    enqueue_network(e, L, n, t);
    wz_launch_repeat = 1;
    F.post_mode = (L.decode_fused ? 1 : 0) | (L.cands_listed ? 2 : 0);   // (wz_debug_post_lane: a replayed graph keeps what it captured)
    enqueue_post(e, L, true, n, t, L.decode_fused, L.cands_listed);
}
// ... with what it launches noted in F, once per key (stamps build): at capture, or at the key's first kernel-by-kernel enqueue
static void enqueue_noted(wz_engine* e, Lane& L, GraphForm& F, int n) {
#if WZ_LANE_STAMPS
    if (!F.noted) g_launch_sink = &F.notes;
    F.noted = true;
#endif
    enqueue_batch(e, L, F, n, nullptr);
#if WZ_LANE_STAMPS
    g_launch_sink = nullptr;
#endif
}

// a split-operand block no kernel took (the load-time check prepared batch 1 only): nothing may run on stale data
static int launch_refusal(wz_engine* e, Lane& L, int n) {
    const int op = L.launch_failed - 1;
    L.launch_failed = 0;
    return wz_set_error(WZ_EFORMAT, "no %s kernel took op %d (%s) at batch %d",
                        e->ops[op].kind == WZ_OP_DWSEP ? "depthwise-separable" : "split-operand", op, e->ops[op].name, n);
}

// The graph of (lane, batch size, resize form): the batch captured, the resize kernel's node found in it where its arguments are this
// batch's descriptors, the graph instantiated.  Built aside: F takes all of it or stays as it was.
static int capture_form(wz_engine* e, Lane& L, int n, GraphForm& F) {
    GraphForm fresh;
    HIPCHK(hipStreamBeginCapture(L.stream, hipStreamCaptureModeThreadLocal));
    L.lone = false;   // (a captured graph is what runs while the other lanes are busy)
    enqueue_noted(e, L, fresh, n);
    HIPCHK(hipStreamEndCapture(L.stream, &fresh.src));
    if (L.launch_failed) return launch_refusal(e, L, n);
    size_t nodes = 0;
    if (hipGraphGetNodes(fresh.src, nullptr, &nodes) == hipSuccess) fresh.nodes = (int)nodes;
    const bool by_value = e->desc_by_value && n <= WZ_DESC_PACK && nodes > 0;
    if (by_value) {
        std::vector<hipGraphNode_t> all(nodes);
        const void* want = pre_launch(e, L, n).func;
        if (hipGraphGetNodes(fresh.src, all.data(), &nodes) == hipSuccess)
            for (size_t k = 0; k < nodes && !fresh.pre_node; ++k) {
                hipGraphNodeType ty;
                hipKernelNodeParams kp;
                if (hipGraphNodeGetType(all[k], &ty) == hipSuccess && ty == hipGraphNodeTypeKernel &&
                    hipGraphKernelNodeGetParams(all[k], &kp) == hipSuccess && kp.func == want)
                    fresh.pre_node = all[k];
            }
        if (!fresh.pre_node) return wz_set_error(WZ_EHIP, "the resize kernel's node was not found in the captured graph");
    }
    HIPCHK(hipGraphInstantiate(&fresh.exec, fresh.src, nullptr, nullptr, 0));
    if (!fresh.pre_node) {   // (a node handle lives as long as the graph it belongs to: without one the graph is not kept)
        (void)hipGraphDestroy(fresh.src);
        fresh.src = nullptr;
    }
    F = std::move(fresh);
    return WZ_OK;
}

// this batch's descriptors into the arguments of the captured resize node, then the replay
static int replay_form(wz_engine* e, Lane& L, int n, GraphForm& F) {
    if (F.pre_node) {
        const WzPreLaunch d = pre_launch(e, L, n);
        F.args.set(nullptr, L.desc.h, n, (int)e->hdr.input_size, L.tptr[input_tensor_index(e)], L.d_desc, d.flags);
        const hipKernelNodeParams kp = d.node_params(F.args);
        HIPCHK(hipGraphExecKernelNodeSetParams(F.exec, F.pre_node, &kp));
    }
    HIPCHK(hipGraphLaunch(F.exec, L.stream));
    return WZ_OK;
}

int run_batch(wz_engine* e, int slot, int n) {
    Lane& L = e->lanes[slot];
    L.key = n | (L.rows ? 1 << 16 : 0);
    GraphForm& F = L.forms[L.key];
    bool graph = e->use_graph;
    if (graph && e->graph_adaptive) {
        // a LONE batch -- nothing in flight on any other lane -- is launched kernel by kernel: the GPU starts on the first kernel while the host issues the
        // other 29 and the batch is done ~7 us sooner; with another lane busy the captured graph is replayed (10 us of host time instead of 84: what
        // keeps one thread ahead of four lanes).  The same launches either way: the rows do not depend on it (tests/test_gpu_variants.py).
        graph = false;
        for (int li = 0; li < e->n_lanes && !graph; ++li)
            if (li != slot && e->lanes[li].done && hipEventQuery(e->lanes[li].done) == hipErrorNotReady) graph = true;
        (void)hipGetLastError();
    }
    // captured and instantiated the first time the key is seen -- also when that first batch itself goes kernel by kernel (adaptive launch): the several
    // ms of capture + instantiation then land on the first batch of a size, not on the first moment another lane happens to be busy
    if (e->use_graph && !F.exec) WZCHK(capture_form(e, L, n, F));
    if (graph) {
        WZCHK(replay_form(e, L, n, F));
    } else {
        L.lone = true;    // kernel by kernel: the other lanes are idle (adaptive launch), or the process runs without graphs (latency schedule, WZ_GRAPH=0)
        enqueue_noted(e, L, F, n);   // (what was launched: also without a captured graph -- WZ_GRAPH=0, one lane)
        L.lone = false;
        HIPCHK(hipGetLastError());
        if (L.launch_failed) {
            (void)hipStreamSynchronize(L.stream);
            return launch_refusal(e, L, n);
        }
    }
    HIPCHK(hipEventRecord(L.done, L.stream));
    L.n = n;
    return WZ_OK;
}

// ------------------------------------------------------------------------------------------------
// lifecycle
// ------------------------------------------------------------------------------------------------
extern "C" int wz_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- the process's schedule (wz_common.h: wz_latency_schedule; include/watsor_hip.h: wz_set_schedule) --------------------------
static std::atomic<int> g_schedule{-1};   // -1: not fixed yet; WZ_SCHEDULE_THROUGHPUT / WZ_SCHEDULE_LATENCY once anything asked
bool wz_latency_schedule() {
    int s = g_schedule.load();
    if (s < 0) {
        const char* env = getenv("WZ_SCHEDULE");
        int want = (env && (env[0] == 'l' || env[0] == 'L')) ? WZ_SCHEDULE_LATENCY : WZ_SCHEDULE_THROUGHPUT;
        int expect = -1;
        g_schedule.compare_exchange_strong(expect, want);
        s = g_schedule.load();
    }
    return s == WZ_SCHEDULE_LATENCY;
}
extern "C" int wz_set_schedule(int schedule) {
    if (schedule != WZ_SCHEDULE_THROUGHPUT && schedule != WZ_SCHEDULE_LATENCY) return wz_set_error(WZ_EINVAL, "wz_set_schedule: unknown schedule %d", schedule);
    int expect = -1;
    if (g_schedule.compare_exchange_strong(expect, schedule) || expect == schedule) return WZ_OK;
    return wz_set_error(WZ_EINVAL, "wz_set_schedule: the launch shapes of this process were already fixed for the %s schedule (set it before the first wz_create)",
                   expect == WZ_SCHEDULE_LATENCY ? "latency" : "throughput");
}
extern "C" int wz_get_schedule(void) { return wz_latency_schedule() ? WZ_SCHEDULE_LATENCY : WZ_SCHEDULE_THROUGHPUT; }

// "0000:c1:00.0" of a device: what /sys/bus/pci/devices/<id>/{numa_node,local_cpulist} are keyed by (watsor_amd/numa.py)
extern "C" int wz_device_pci_bus_id(int device, char* buf, int buflen) {
    if (!buf || buflen < 16) return wz_set_error(WZ_EINVAL, "wz_device_pci_bus_id: buffer of at least 16 bytes expected");
    if (hipDeviceGetPCIBusId(buf, buflen, device) != hipSuccess) {
        (void)hipGetLastError();
        return wz_set_error(WZ_ENODEV, "no HIP device %d", device);
    }
    return WZ_OK;
}

extern "C" int wz_device_name_of(int device, char* buf, int buflen) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, device) != hipSuccess) return wz_set_error(WZ_ENODEV, "no HIP device %d", device);
    snprintf(buf, buflen, "%s (%s)", p.name, p.gcnArchName);
    return WZ_OK;
}

extern "C" const char* wz_last_error(void) { return g_err; }

// The Inception op kinds and the channel-slice outputs (format 12): every bound the kernels rely on, since they index by these fields
// alone.  Returns false for a malformed op.
static bool slice_op_ok(const wz_engine* e, const WzOpDesc& op) {
    const WzBlobHeader& h = e->hdr;
    const bool is_new = op.kind == WZ_OP_POOL || op.kind == WZ_OP_STEM7;
    if (!is_new && !(op.kind == WZ_OP_CONV && op.dst_c != 0)) return true;   // (the MobileNet ops: checked as before)
    if (op.out_mode != WZ_OUT_ACT || op.dst < 0 || op.res >= 0 || op.dst == op.src) return false;
    const WzTensorDesc& in = e->tensors[op.src];
    const WzTensorDesc& out = e->tensors[op.dst];
    const int cs = op.dst_c ? op.dst_c : op.cout;
    // the slice: whole 16-byte channel groups, inside the tensor, which has the op's output map
    if (op.dst_c < 0 || cs != out.c || op.dst_coff < 0 || op.dst_coff % 8 != 0 || op.cout % 8 != 0 || op.dst_coff + op.cout > cs ||
        out.h != op.hout || out.w != op.wout || (out.flags & WZ_TENSOR_HP))
        return false;
    if (in.h != op.hin || in.w != op.win || op.stride < 1 || op.stride > 2 || op.hout != (op.hin + op.stride - 1) / op.stride ||
        op.wout != (op.win + op.stride - 1) / op.stride)
        return false;
    if (op.kind == WZ_OP_POOL)
        return op.ksize == 3 && op.cin == op.cout && in.c == op.cin && !(in.flags & WZ_TENSOR_HP) && op.pad_t >= 0 && op.pad_t <= 1 &&
               op.pad_l >= 0 && op.pad_l <= 1 && (op.flags & ~(int64_t)WZ_OPF_POOL_AVG) == 0;
    if (op.kind == WZ_OP_STEM7) {
        const uint64_t wbytes = h.precision == 32 ? 49ull * 3 * 64 * 4 : 64ull * 7 * 32 * 2;
        return op.ksize == 7 && op.stride == 2 && op.cin == 3 && op.cout == 64 && in.c == 4 && op.src == e->ops[0].src &&
               op.pad_t >= 0 && op.pad_t <= 3 && op.pad_l >= 0 && op.pad_l <= 3 &&
               ((in.flags & WZ_TENSOR_HP) != 0) == (h.precision == 32) && (h.precision == 32 || (op.kc == 7 && op.n_pad == 64)) &&
               op.w_off >= 0 && (uint64_t)op.w_off + wbytes <= h.weights_bytes && op.b_off >= 0 && (uint64_t)op.b_off + 256 <= h.weights_bytes;
    }
    return in.c == op.cin;   // a sliced conv reads a whole tensor
}

static int load_blob(wz_engine* e, const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return wz_set_error(WZ_ENOENT, "engine file not found: %s", path);
    fseek(f, 0, SEEK_END);
    long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz < (long)sizeof(WzBlobHeader)) {
        fclose(f);
        return wz_set_error(WZ_EFORMAT, "engine file %s is truncated", path);
    }
    e->blob.resize(sz);
    size_t rd = fread(e->blob.data(), 1, sz, f);
    fclose(f);
    if (rd != (size_t)sz) return wz_set_error(WZ_EFORMAT, "short read on %s", path);
    memcpy(&e->hdr, e->blob.data(), sizeof(WzBlobHeader));
    const WzBlobHeader& h = e->hdr;
    if (h.magic != WZ_MAGIC) return wz_set_error(WZ_EFORMAT, "%s is not an mi355x engine (bad magic)", path);
    if (h.version == WZ_FORMAT_VERSION && (h.resize_mode > 1 || h.post_flags > 1))
        return wz_set_error(WZ_EFORMAT, "%s: unknown resize mode %u / post-processing flags %u", path, h.resize_mode, h.post_flags);
    if (h.version != WZ_FORMAT_VERSION)
        return wz_set_error(WZ_EFORMAT, "%s: engine format %u, runtime expects %u -- rebuild it with watsor_amd.engine",
                       path, h.version, WZ_FORMAT_VERSION);
    if (h.total_bytes != (uint64_t)sz || (h.precision != 16 && h.precision != 32) || h.max_total > WZ_MAX_DETECTIONS || h.max_total < 1 ||
        h.num_classes > 4096 || h.n_ops == 0 || h.weights_off + h.weights_bytes > (uint64_t)sz ||
        h.tensors_off + (uint64_t)h.n_tensors * sizeof(WzTensorDesc) > (uint64_t)sz ||
        h.ops_off + (uint64_t)h.n_ops * sizeof(WzOpDesc) > (uint64_t)sz ||
        h.anchors_off + (uint64_t)h.num_anchors * 16 > (uint64_t)sz)
        return wz_set_error(WZ_EFORMAT, "%s: inconsistent engine header", path);
    e->tensors = reinterpret_cast<const WzTensorDesc*>(e->blob.data() + h.tensors_off);
    e->ops = reinterpret_cast<const WzOpDesc*>(e->blob.data() + h.ops_off);
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        const WzOpDesc& op = e->ops[i];
        if (op.kind < WZ_OP_STEM || op.kind > WZ_OP_DWSEP)   // (an unknown kind would otherwise run as a conv)
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s) has kind %d, which this runtime does not know", path, i, op.name, op.kind);
        if (op.src < 0 || op.src >= (int)h.n_tensors || op.dst >= (int)h.n_tensors || op.res >= (int)h.n_tensors ||
            (op.out_mode == WZ_OUT_ACT && op.dst < 0) || op.w_off < 0 || (uint64_t)op.w_off >= h.weights_bytes ||
            (op.kind == WZ_OP_CONV && (op.n_pad % 32 != 0 || op.cin % 8 != 0 || op.n_pad < op.cout ||
                                       (op.out_mode == WZ_OUT_ACT && op.cout % 8 != 0) ||
                                       (op.ksize != 1 && op.ksize != 3) ||
                                       (op.out_mode == WZ_OUT_HEAD && (op.n_box % 4 != 0 || op.n_box <= 0 || op.n_box >= op.cout)))) ||
            (op.kind == WZ_OP_DW && op.cin % 8 != 0) ||
            (op.kind == WZ_OP_MBCONV &&
             (op.dst < 0 || op.cmid < 8 || op.cmid % 8 != 0 || op.cmid_pad != (op.cmid + 31) / 32 * 32 ||
              op.kc != op.cmid_pad / 32 || op.n_pad % 32 != 0 || op.n_pad < op.cout || op.cout % 8 != 0 ||
              op.wd_off < 0 || (uint64_t)op.wd_off >= h.weights_bytes || op.bd_off < 0 ||
              (uint64_t)op.bd_off >= h.weights_bytes || op.stride < 1 || op.stride > 2 ||
              (op.cin0 != 0 && (op.cin0 % 8 != 0 || op.kc0 != (op.cin0 + 31) / 32 || op.nmid_pad % 16 != 0 ||
                                op.nmid_pad < op.cmid || op.we_off < 0 || (uint64_t)op.we_off >= h.weights_bytes ||
                                op.be_off < 0 || (uint64_t)op.be_off >= h.weights_bytes)))))
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s) is malformed", path, i, op.name);
        if (!slice_op_ok(e, op))
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): malformed pool / 7x7 stem / channel-slice output", path, i, op.name);
        if (op.dst2 != 0) {
            const WzTensorDesc* t2 = (op.dst2 > 0 && op.dst2 <= (int64_t)h.n_tensors) ? &e->tensors[op.dst2 - 1] : nullptr;
            if (op.kind != WZ_OP_MBCONV || !t2 || op.cin0 <= 0 || t2->h != op.hin || t2->w != op.win ||
                t2->c != op.cmid || (t2->flags & WZ_TENSOR_HP) || op.dst2 - 1 == op.dst || op.dst2 - 1 == op.src)
                return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): malformed second output", path, i, op.name);
        }
        if (op.kind == WZ_OP_MBCONV && h.precision != 16)
            return wz_set_error(WZ_EFORMAT, "%s: fused blocks exist for the fp16 engine only", path);
        if (h.precision == 32 && ((op.kind == WZ_OP_CONV && op.cin % 4 != 0) || (op.kind == WZ_OP_DW && op.cin % 4 != 0)))
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s) is malformed", path, i, op.name);
        if (op.kind == WZ_OP_MBCONV && (op.flags & WZ_OPF_HP)) {
            if (!(e->tensors[op.src].flags & WZ_TENSOR_HP) || (op.res >= 0 && op.res != op.src) ||
                ((op.flags & WZ_OPF_HP_OUT) != 0) != ((e->tensors[op.dst].flags & WZ_TENSOR_HP) != 0) ||
                ((op.flags & WZ_OPF_DUP_OUT) && ((op.flags & WZ_OPF_HP_OUT) || e->tensors[op.dst].c != 2 * op.cout)) ||
                (!(op.flags & WZ_OPF_DUP_OUT) && e->tensors[op.dst].c != op.cout) ||
                op.we_lo_off <= 0 || (uint64_t)op.we_lo_off >= h.weights_bytes || op.w_lo_off <= 0 ||
                (uint64_t)op.w_lo_off >= h.weights_bytes || (op.stem && e->tensors[op.src].c != 4))
                return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): malformed split-operand block", path, i, op.name);
        } else if ((op.kind == WZ_OP_STEM || op.kind == WZ_OP_STEM7) && h.precision == 32 && (e->tensors[op.src].flags & WZ_TENSOR_HP) &&
                   !(op.dst >= 0 && (e->tensors[op.dst].flags & WZ_TENSOR_HP))) {
            // the fp32 program's stem reads the network input as a hi + lo pair (wz_k_stem_f32)
        } else if ((e->tensors[op.src].flags & WZ_TENSOR_HP) || (op.dst >= 0 && (e->tensors[op.dst].flags & WZ_TENSOR_HP)) ||
                   (op.res >= 0 && (e->tensors[op.res].flags & WZ_TENSOR_HP))) {
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s) touches a pair tensor but is not a split-operand block", path, i, op.name);
        } else if (op.kind == WZ_OP_DWSEP) {
            // every bound the kernel indexes by: the tensors it reads and writes, both weight blocks; the shapes it covers are
            // op_kernel_check's, evaluated with the predicate of the launch, so that an uncovered shape never reaches run_batch
            const WzTensorDesc& in = e->tensors[op.src];
            const WzTensorDesc* out = op.dst >= 0 ? &e->tensors[op.dst] : nullptr;
            const uint64_t wb = h.weights_bytes;
            if (h.precision != 16 || !out || op.out_mode != WZ_OUT_ACT || op.res >= 0 || op.dst_c != 0 || op.dst_coff != 0 || op.dst2 != 0 ||
                op.flags != 0 || op.ksize != 3 || op.act != WZ_ACT_RELU6 || op.dst == op.src || op.cin < 8 || op.cout < 8 || op.kc < 1 ||
                op.n_pad < op.cout || in.c != op.cin || in.h != op.hin || in.w != op.win || out->c != op.cout || out->h != op.hout ||
                out->w != op.wout || op.wd_off < 0 || (uint64_t)op.wd_off + 9ull * op.cin * 2 > wb || op.bd_off < 0 ||
                (uint64_t)op.bd_off + 4ull * op.cin > wb || (uint64_t)op.w_off + 64ull * op.n_pad * op.kc > wb || op.b_off < 0 ||
                (uint64_t)op.b_off + 4ull * op.n_pad > wb)
                return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): malformed depthwise-separable layer", path, i, op.name);
        } else if (op.kind == WZ_OP_MBCONV && op.stem) {
            if (e->tensors[op.src].c != 4 || op.cin0 != 32 || op.kc0 != 1 || (e->tensors[op.src].h + 1) / 2 != op.hin ||
                (e->tensors[op.src].w + 1) / 2 != op.win)
                return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): malformed stem fusion", path, i, op.name);
        }
        WZCHK(op_kernel_check(e, op, path));   // the op is well-formed: is there a kernel for its shape?
    }
    return WZ_OK;
}

// Every synchronous copy and fill of a product path: issued on lane 0's stream and waited for there -- not hipMemcpy / hipMemset,
// which ride the null stream and make ROCclr open a hardware queue for it that a lane may then have to share (a process that uses
// only the product ABI never creates that queue).  Waits for whatever lane 0 has in flight, the source is free on return.
static hipError_t lane0_copy(wz_engine* e, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    const hipError_t err = hipMemcpyAsync(dst, src, bytes, kind, e->stream);
    return err == hipSuccess ? hipStreamSynchronize(e->stream) : err;
}
hipError_t lane0_fill(wz_engine* e, void* dst, int value, size_t bytes) {
    const hipError_t err = hipMemsetAsync(dst, value, bytes, e->stream);
    return err == hipSuccess ? hipStreamSynchronize(e->stream) : err;
}

// what the environment says about an engine for frames up to max_width wide (the product library reads WZ_GRAPH, WZ_LANES, WZ_STREAMS and
// the schedule; the development library its knobs as well), and the device's compute units
static void read_options(wz_engine* e, int max_width) {
    const char* env;
    e->no_reuse = (env = wz_dev_getenv("WZ_NO_BUFFER_REUSE")) && atoi(env) != 0;
    // WZ_GRAPH=0|1 decides when set.  Unset: captured graphs under the throughput schedule WHILE ANOTHER LANE IS BUSY (a batch is handed over in 10.5 us: one
    // thread keeps four lanes fed; a batch that finds the other lanes idle goes kernel by kernel: run_batch), kernel-by-kernel launches under the LATENCY schedule -- the GPU starts on the first kernel while the host still issues the rest, and a lone
    // batch is done 7 us sooner (0.380 -> 0.372 ms at batch 8, 0.2915 -> 0.2865 at batch 1; 84 us of host time per batch instead of 10, and 2 - 4 % of the
    // saturated throughput: profiles/r05_submit_probe.txt)
    env = getenv("WZ_GRAPH");
    if (env && !env[0]) env = nullptr;   // (set but empty = not set)
    e->use_graph = env ? atoi(env) != 0 : !wz_latency_schedule();
    e->graph_adaptive = e->use_graph && !env;   // (throughput schedule, nothing said: graphs while the lanes are busy, kernel by kernel for a lone batch)
    e->use_splitk = !((env = wz_dev_getenv("WZ_SPLITK")) && atoi(env) == 0);
    e->defer_heads = !((env = wz_dev_getenv("WZ_DEFER_HEADS")) && atoi(env) == 0);
    e->fuse_decode = !((env = wz_dev_getenv("WZ_FUSE_DECODE")) && atoi(env) == 0);
    e->conv_wide = !((env = wz_dev_getenv("WZ_CONV_WIDE")) && atoi(env) == 0);
    e->desc_zero_copy = !((env = wz_dev_getenv("WZ_DESC_COPY")) && atoi(env) != 0);
    e->desc_by_value = !((env = wz_dev_getenv("WZ_DESC_ARGS")) && atoi(env) == 0);
    e->pre_rows = (env = wz_dev_getenv("WZ_PRE_ROWS")) ? atoi(env) != 0 : e->pre_rows;
    // WZ_SCHEDULE=latency: every page-locked frame is read in place -- a lone batch is done sooner without the staging copy in front of it
    // (640x480, batch 8: 0.505 against 0.575 ms) although the waiting workgroups cost frames/s with four lanes in flight (29.7 k against 34 k)
    if (wz_latency_schedule()) e->host_read = 1;
    e->host_read = (env = wz_dev_getenv("WZ_HOST_READ")) ? atoi(env) : e->host_read;
    e->pre_rows_lds = (int)wz_preprocess_rows_lds(max_width);
    if (e->pre_rows_lds > 60 * 1024) e->pre_rows = false, e->host_read = 0;   // (frames wider than ~6 800 pixels need more LDS than a launch gets by default: the per-pixel form, staged)
    e->wide_T = (env = wz_dev_getenv("WZ_WIDE_T")) ? atoi(env) : 0;
    e->wide_min_m = (env = wz_dev_getenv("WZ_WIDE_MIN_M")) ? atoi(env) : 1;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        e->num_cus = cus;
    e->wide_cus = wz_latency_schedule() ? e->num_cus : e->num_cus / 2;
    if ((env = wz_dev_getenv("WZ_WIDE_CUS")) && atoi(env) > 0) e->wide_cus = atoi(env);
    if ((env = getenv("WZ_LANES")) && atoi(env) >= 1 && atoi(env) <= WZ_SLOTS) e->n_lanes = atoi(env);
    if ((env = getenv("WZ_STREAMS")) && atoi(env) >= 1 && atoi(env) <= WZ_SLOTS) e->n_streams = atoi(env);
    if (e->n_streams > e->n_lanes) e->n_streams = e->n_lanes;
}

// A lane's descriptors in device memory -- in the stamps build behind its launch blocks and the resize kernel's block: one block, carved
static size_t lane_parts(Lane& L, const void* base, size_t nb) {
    Carve c(base);
#if WZ_LANE_STAMPS
    L.d_stamps = c.take<unsigned long long>((size_t)WZ_STAMP_SLOTS * WZ_STAMP_WORDS);
    L.d_stamps_pre = c.take<unsigned long long>(WZ_STAMP_PRE_BYTES / 8);
#endif
    L.d_desc = c.take<WzFrameDesc>(nb);
    return c.bytes();
}

// Lane li of a new engine, whose streams exist: every block the lane owns, WzPostBuffers as views of them, its event
static int build_lane(wz_engine* e, int li) {
    Lane& L = e->lanes[li];
    const WzBlobHeader& h = e->hdr;
    const size_t nb = (size_t)e->max_batch;
    // More lanes than streams (WZ_STREAMS, default 4 = what this stack runs side by side): lane i rides the stream of lane
    // i mod streams, with buffers, graph and host blocks of its own -- the stream always has the next batch queued behind the one
    // it is running, so the host's turnaround between a batch's end and the next submit is not idle time on that queue.
    if (li >= e->n_streams) L.stream = e->lanes[li % e->n_streams].stream;   // (the first n_streams lanes own theirs)
    // activation buffers: one per slot (tensors with disjoint lifetimes share), or one per tensor
    std::vector<size_t> buf_bytes(e->no_reuse ? h.n_tensors : h.n_slots, 0);
    for (uint32_t i = 0; i < h.n_tensors; ++i) {
        size_t& b = buf_bytes[e->no_reuse ? i : (uint32_t)e->tensors[i].slot];
        b = std::max(b, nb * tensor_frame_bytes(e, i) + 256);
    }
    L.bufs.resize(buf_bytes.size());
    for (size_t k = 0; k < buf_bytes.size(); ++k) HIPCHK(L.bufs[k].alloc(buf_bytes[k]));
    L.tptr.assign(h.n_tensors, nullptr);
    for (uint32_t i = 0; i < h.n_tensors; ++i) L.tptr[i] = reinterpret_cast<half_t*>(L.bufs[e->no_reuse ? i : (uint32_t)e->tensors[i].slot].p);
    HIPCHK(L.d_box_enc.alloc(nb * h.num_anchors * 4));
    HIPCHK(L.d_logits.alloc(nb * h.num_anchors * h.num_classes));
    HIPCHK(L.d_ws.alloc(e->ws_bytes / sizeof(float)));
    HIPCHK(L.d_frames.alloc(e->frame_stride * nb));
    WzPostBuffers& pb = L.post;
    pb.box_enc = L.d_box_enc;
    pb.logits = L.d_logits;
    pb.anchors = e->d_anchors;
    HIPCHK(L.d_boxes.alloc(nb * h.num_anchors * 4));
    HIPCHK(L.d_valid.alloc(nb * h.num_anchors));
    HIPCHK(L.d_post_scratch.alloc(e->post_scratch_bytes / 4));
    pb.boxes = L.d_boxes;
    pb.valid = L.d_valid;
    pb.hint = L.d_post_scratch;
    {   // first band of the NMS kernel: start at score 0.25 until the frame slot has a history
        const uint32_t bin0 = 0x3E800000u >> 20;
        std::vector<uint32_t> hint0(nb, bin0);
        HIPCHK(lane0_copy(e, pb.hint, hint0.data(), hint0.size() * 4, hipMemcpyHostToDevice));
        pb.hint_logit = reinterpret_cast<float*>(pb.hint + nb);
        uint32_t sbits = bin0 << 20;
        float s0;
        memcpy(&s0, &sbits, 4);
        const float l0 = logf(s0 / (1.0f - s0));   // wz_logit_floor(bin0), k_post.hip
        std::vector<float> hl0(nb, l0 - 0.01f - 1e-3f * fabsf(l0));
        HIPCHK(lane0_copy(e, pb.hint_logit, hl0.data(), hl0.size() * 4, hipMemcpyHostToDevice));
        pb.cbits = reinterpret_cast<uint32_t*>(pb.hint_logit + nb);
        HIPCHK(lane0_fill(e, pb.cbits, 0, nb * ((h.num_anchors * h.num_classes + 31) >> 5) * 4));
    }
    HIPCHK(L.d_det_boxes.alloc(nb * h.max_total * 4));
    HIPCHK(L.d_det_scores.alloc(nb * h.max_total));
    HIPCHK(L.d_det_classes.alloc(nb * h.max_total));
    HIPCHK(L.d_det_num.alloc(nb));
    HIPCHK(L.d_dbg.alloc(nb * 16));
    HIPCHK(lane0_fill(e, L.d_dbg, 0, nb * 16 * 8));
    pb.det_boxes = L.d_det_boxes;
    pb.det_scores = L.d_det_scores;
    pb.det_classes = L.d_det_classes;
    pb.det_num = L.d_det_num;
    pb.dbg = L.d_dbg;
    HIPCHK(L.desc.alloc(nb, false));
    HIPCHK(L.d_parts.alloc(lane_parts(L, nullptr, nb)));
    lane_parts(L, L.d_parts, nb);
#if WZ_LANE_STAMPS
    {   // the launch blocks and the resize kernel's block: every pair starts as (entry = max, exit = 0)
        std::vector<unsigned long long> init((size_t)(WZ_STAMP_SLOTS + 1) * WZ_STAMP_WORDS, 0ull);
        for (size_t k = 0; k < init.size(); k += WZ_STAMP_WORDS)
            for (int j = 0; j < 64; ++j) init[k + WZ_STAMP_ENTRY + j] = ~0ull;
        HIPCHK(lane0_copy(e, L.d_parts, init.data(), init.size() * 8, hipMemcpyHostToDevice));
        const size_t host_words = (size_t)(WZ_STAMP_SLOTS + 1 + nb) * 2;
        HIPCHK(L.hstamps.alloc(host_words));
        memset(L.hstamps.h, 0, host_words * 8);
    }
#endif
    pb.stamps = L.d_stamps;
    pb.stamps_pre = L.d_stamps_pre;
    pb.stamps_host = nullptr;
    pb.stamps_n = 0;
    pb._stamps_pad = 0;
    HIPCHK(L.hrows.alloc((size_t)WZ_MAX_DETECTIONS * nb));
    HIPCHK(L.hpass.alloc((size_t)WZ_MAX_DETECTIONS * nb));
    HIPCHK(L.hstatus.alloc(nb));
    memset(L.hstatus.h, 0, sizeof(uint32_t) * nb);
    HIPCHK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    return WZ_OK;
}

// the engine on its device: streams, the engine-wide blocks, the lanes, the stage names
static int build_engine(wz_engine* e) {
    const WzBlobHeader& h = e->hdr;
    HIPCHK(hipSetDevice(e->device));
    char nm[256];
    wz_device_name_of(e->device, nm, sizeof(nm));
    e->name = nm;
    wz_post_init();
    network_prepare(e);   // kernel attributes of the fused-block kernels, on THIS device; what the op list says about every op

    // the lanes' streams before anything is copied: the set-up copies below ride lane 0's (lane0_copy)
    for (int li = 0; li < e->n_streams; ++li) {
        HIPCHK(hipStreamCreateWithFlags(&e->lanes[li].stream, hipStreamNonBlocking));
        e->lanes[li].owns_stream = true;
    }
    e->stream = e->lanes[0].stream;

    HIPCHK(e->d_weights.alloc(h.weights_bytes));
    HIPCHK(lane0_copy(e, e->d_weights, e->blob.data() + h.weights_off, h.weights_bytes, hipMemcpyHostToDevice));
    const char* env;
    if ((env = wz_dev_getenv("WZ_MB_DEBUG")) && atoi(env) != 0) {
        HIPCHK(e->d_mbdbg.alloc((size_t)h.n_ops * 16));
        HIPCHK(lane0_fill(e, e->d_mbdbg, 0, (size_t)h.n_ops * 16 * 8));
        e->mb_groups.assign(h.n_ops, 0);
    }
    HIPCHK(e->d_zeros.alloc(4096 / sizeof(half_t)));
    HIPCHK(lane0_fill(e, e->d_zeros, 0, 4096));
    HIPCHK(e->d_anchors.alloc((size_t)h.num_anchors * 4));
    HIPCHK(lane0_copy(e, e->d_anchors, e->blob.data() + h.anchors_off, (size_t)h.num_anchors * 16, hipMemcpyHostToDevice));
    e->frame_stride = ((size_t)e->max_w * e->max_h * 3 + 255) & ~(size_t)255;
    e->ws_bytes = std::max<size_t>((size_t)64 << 20, (size_t)e->max_batch * ((size_t)32 << 20));

    e->pc.num_anchors = h.num_anchors;
    e->pc.num_classes = h.num_classes;
    e->pc.max_total = h.max_total;
    e->pc.max_per_class = h.max_per_class;
    e->pc.score_thr = h.score_threshold;
    e->pc.iou_thr = h.iou_threshold;
    e->pc.scale_y = h.scale_y; e->pc.scale_x = h.scale_x; e->pc.scale_h = h.scale_h; e->pc.scale_w = h.scale_w;
    e->pc.clip_after = (h.post_flags & WZ_POSTF_CLIP_AFTER) ? 1 : 0;
    e->pc._pad = 0;
    e->post_scratch_bytes = (size_t)e->max_batch * (2 + ((h.num_anchors * h.num_classes + 31) >> 5)) * 4;   // hint, hint_logit, cbits

    for (uint32_t i = 0; i < h.n_tensors; ++i)
        if (e->tensors[i].slot < 0 || e->tensors[i].slot >= (int)h.n_slots) return wz_set_error(WZ_EFORMAT, "tensor %u has a bad slot", i);
    for (int li = 0; li < e->n_lanes; ++li) WZCHK(build_lane(e, li));

    e->h_cams.resize(WZ_MAX_CAMS);
    memset(e->h_cams.data(), 0, sizeof(WzCamFilter) * WZ_MAX_CAMS);
    e->cam_sat.resize(WZ_MAX_CAMS);
    HIPCHK(e->d_cams.alloc(WZ_MAX_CAMS));
    HIPCHK(lane0_fill(e, e->d_cams, 0, sizeof(WzCamFilter) * WZ_MAX_CAMS));
    HIPCHK(e->d_tmp_rows.alloc(WZ_MAX_DETECTIONS));
    HIPCHK(e->d_tmp_pass.alloc(WZ_MAX_DETECTIONS));

    e->stage_names = {"(empty)", "h2d_descriptors", "preprocess"};
    for (uint32_t i = 0; i < h.n_ops; ++i) {
        e->stage_names.push_back(e->ops[i].name);   // stage_slots(op) names per op: enqueue_network marks as many
        for (int k = 1; k < stage_slots(e->ops[i]); ++k) e->stage_names.push_back(std::string(e->ops[i].name) + "#splitk_reduce");
    }
    for (const char* name : {"heads#big_convs", "heads#small_convs", "heads#splitk_reduce", "post/decode", "post/nms", "post/rows"})
        e->stage_names.push_back(name);
    return sync_all(e);
}

extern "C" int wz_create(const char* engine_path, int device, int max_batch, int max_width, int max_height,
                         wz_engine_t** out) {
    if (!engine_path || !out || max_batch < 1 || max_batch > 4095 || max_width < 1 || max_height < 1)
        return wz_set_error(WZ_EINVAL, "wz_create: bad argument");
    *out = nullptr;
    wz_engine* e = new wz_engine();
    int rc = load_blob(e, engine_path);
    const int ndev = rc == WZ_OK ? wz_device_count() : 0;
    if (rc == WZ_OK && (device < 0 || device >= ndev)) rc = wz_set_error(WZ_ENODEV, "HIP device %d not present (%d visible)", device, ndev);
    if (rc == WZ_OK) {
        e->device = device;
        e->max_batch = max_batch;
        e->max_w = max_width;
        e->max_h = max_height;
        read_options(e, max_width);
        rc = build_engine(e);
    }
    if (rc != WZ_OK) {   // the one failure exit: whatever exists by now frees itself
        wz_destroy(e);
        return rc;
    }
    *out = e;
    return WZ_OK;
}

int sync_all(wz_engine* e) {
    for (int li = 0; li < e->n_lanes; ++li)
        if (e->lanes[li].stream) HIPCHK(hipStreamSynchronize(e->lanes[li].stream));
    return WZ_OK;
}

// Every block frees itself with the engine (wz_engine.h); what is destroyed here by hand is what has no owner type: the lanes' events and
// streams.  A lane's graphs go before the stream they were launched on; a lane that rides another lane's stream destroys none.
extern "C" void wz_destroy(wz_engine_t* e) {
    if (!e) return;
    if (e->lanes[0].stream) {   // (nothing is made on the device before the first stream)
        (void)hipSetDevice(e->device);
        (void)sync_all(e);
    }
    for (Lane& L : e->lanes) {
        L.forms.clear();
        if (L.done) (void)hipEventDestroy(L.done);
        if (L.stream && L.owns_stream) (void)hipStreamDestroy(L.stream);
    }
    delete e;
}

extern "C" const char* wz_device_name(wz_engine_t* e) { return e ? e->name.c_str() : ""; }

// ------------------------------------------------------------------------------------------------
// the hot call
// ------------------------------------------------------------------------------------------------
// Why a format word (include/watsor_hip.h: a base format in bits 0-7 | WZ_CSP_BT709 | WZ_RANGE_FULL) is not taken at this size, or
// nullptr when it is.  The one place that knows the rules: wz_frame_bytes -- by which every frame is sized and checked -- is 0
// exactly where this gives a reason.
const char* fmt_refusal(int w, int h, int fmt) {
    if (w < 1 || h < 1) return "width and height must be positive";
    if (fmt & ~(WZ_FMT_BASE_MASK | WZ_CSP_BT709 | WZ_RANGE_FULL)) return "unknown flag bits in the format word";
    const int base = fmt & WZ_FMT_BASE_MASK;
    const bool ten = base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10;   // 10-bit 4:2:0: a 16-bit word per sample
    if (base > WZ_FMT_BGR24 && !ten) return "unknown base format";
    const bool yuv = base == WZ_FMT_NV12 || base == WZ_FMT_I420 || base == WZ_FMT_YUYV422 || base == WZ_FMT_UYVY422 || ten;
    if (!yuv && (fmt & (WZ_CSP_BT709 | WZ_RANGE_FULL))) return "WZ_CSP_BT709 / WZ_RANGE_FULL apply to the YUV formats only, not to RGB24, BGR24 or GRAY8";
    if ((base == WZ_FMT_NV12 || base == WZ_FMT_I420) && ((w | h) & 1)) return "NV12 / I420 need even sides";
    if (ten && ((w | h) & 1)) return "P010 / YUV420P10 need even sides";
    if ((base == WZ_FMT_YUYV422 || base == WZ_FMT_UYVY422) && (w & 1)) return "YUYV422 / UYVY422 need an even width";
    return nullptr;
}
extern "C" uint64_t wz_frame_bytes(int w, int h, int fmt) {
    if (fmt_refusal(w, h, fmt)) return 0;
    const uint64_t px = (uint64_t)w * h;
    switch (fmt & WZ_FMT_BASE_MASK) {
        case WZ_FMT_RGB24: case WZ_FMT_BGR24: return px * 3;
        case WZ_FMT_P010: case WZ_FMT_YUV420P10: return px * 3;   // 2 bytes a sample, 1.5 samples a pixel: RGB24's size
        case WZ_FMT_NV12: case WZ_FMT_I420: return px * 3 / 2;
        case WZ_FMT_YUYV422: case WZ_FMT_UYVY422: return px * 2;
        default: return px;   // WZ_FMT_GRAY8
    }
}

int fill_desc(wz_engine* e, int slot, int n, const uint8_t* const* d_rgb, const int* w, const int* h, const int* fmt, const int* cam) {
    WZCHK(batch_refusal(e, slot, n));
    const float size = (float)e->hdr.input_size;
    e->lanes[slot].bound_idx.clear();
    e->lanes[slot].tile.tiled = 0;
    for (int i = 0; i < n; ++i) {
        const int pf = fmt ? fmt[i] : WZ_FMT_RGB24;
        const int c = cam ? cam[i] : -1;
        WZCHK(frame_refusal(e, "frame", i, d_rgb[i], w[i], h[i], pf, c, FC_PTR | FC_FMT | FC_CAM_ID | FC_CAM_FILTER));
        WzFrameDesc& d = e->lanes[slot].desc.h[i];
        d.rgb = d_rgb[i];
        d.w = w[i];
        d.h = h[i];
        d.scale_x = (float)w[i] / size;   // CalculateResizeScale(in, out, align_corners=false)
        d.scale_y = (float)h[i] / size;
        d.cam = c < 0 ? -1 : c;
        d.fmt = pf;
    }
    return WZ_OK;
}

extern "C" int wz_submit_device_fmt(wz_engine_t* e, int slot, int n, const uint8_t* const* d_rgb, const int* w,
                                    const int* h, const int* fmt, const int* cam) {
    if (!e || !d_rgb || !w || !h) return wz_set_error(WZ_EINVAL, "wz_submit_device: null argument");
    WZCHK(batch_refusal(e, slot, n, BC_SLOT));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->lanes[slot].done));   // the lane's previous batch has fully drained
    WZCHK(fill_desc(e, slot, n, d_rgb, w, h, fmt, cam));
    e->lanes[slot].rows = e->pre_rows && rows_fit(e, n, w, fmt);
    return run_batch(e, slot, n);
}
extern "C" int wz_submit_device(wz_engine_t* e, int slot, int n, const uint8_t* const* d_rgb, const int* w,
                                const int* h, const int* cam) {
    return wz_submit_device_fmt(e, slot, n, d_rgb, w, h, nullptr, cam);
}

extern "C" int wz_wait(wz_engine_t* e, int slot) {
    if (!e || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_wait: bad argument");
    HIPCHK(hipEventSynchronize(e->lanes[slot].done));
    return WZ_OK;
}

// after a lane's rows were handed over: did the NMS kernel flag one of its frames?  (clip-after-NMS engines only; k_post.hip: wz_k_nms)
static int lane_status(wz_engine* e, int slot) {
    const Lane& L = e->lanes[slot];
    for (int i = 0; i < L.n; ++i)
        if (L.hstatus.h[i])
            return wz_set_error(WZ_EINCOMPLETE, "frame %d of the batch on lane %d: more than %d selected boxes lie entirely outside the image, "
                                           "its rows may be incomplete", i, slot, WZ_NMS_KEEP_MAX - (int)e->hdr.max_total);
    return WZ_OK;
}

// What a lane hands over.  A tiled or gated batch: its FRAMES' merged rows, one block per frame -- tile.tiled of them, whatever L.n says
// (the tiles that ran; none: 0; lane_status still looks at every tile).
struct LaneResult { int n; const wz_detection_t* rows; const uint8_t* pass; };
static LaneResult lane_result(const Lane& L) {
    return L.tile.tiled ? LaneResult{L.tile.tiled, L.tile.trows.h, L.tile.tpass.h} : LaneResult{L.n, L.hrows.h, L.hpass.h};
}

extern "C" const wz_detection_t* wz_slot_rows(wz_engine_t* e, int slot) {
    if (!e || slot < 0 || slot >= e->n_lanes) return nullptr;
    return lane_result(e->lanes[slot]).rows;
}

extern "C" int wz_collect(wz_engine_t* e, int slot, wz_detection_t* const* out, uint8_t* const* pass) {
    WZCHK(wz_wait(e, slot));
    const LaneResult r = lane_result(e->lanes[slot]);
    for (int i = 0; i < r.n; ++i) {
        if (out && out[i])
            memcpy(out[i], r.rows + (size_t)i * WZ_MAX_DETECTIONS, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS);
        if (pass && pass[i]) memcpy(pass[i], r.pass + (size_t)i * WZ_MAX_DETECTIONS, WZ_MAX_DETECTIONS);
    }
    return lane_status(e, slot);
}

extern "C" int wz_num_slots(wz_engine_t* e) { return e ? e->n_lanes : 0; }

extern "C" int wz_graph_nodes(wz_engine_t* e, int slot) {
    if (!e || slot < 0 || slot >= e->n_lanes) return 0;
    const Lane& L = e->lanes[slot];
    const auto it = L.forms.find(L.key);
    return it == L.forms.end() ? 0 : it->second.nodes;
}

extern "C" int wz_sync(wz_engine_t* e) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_sync: null engine");
    return sync_all(e);
}

// The host frames of a batch going onto lane L, placed: ptr[i] comes in as frame i's host address and leaves as where the device finds
// the frame -- the frame itself, read in place, where `may_read` and read_in_place allow it and the device sees it (*in_place: one is), else its
// copy in the lane's staging area.  entries: the frames are these entries of the frame table (null: plain pointers, looked up).
static int place_frames(wz_engine* e, Lane& L, int n, const uint8_t** ptr, const int* w, const int* h, const int* fmt, const int32_t* entries,
                        bool may_read, bool* in_place) {
    *in_place = false;
    for (int i = 0; i < n; ++i) {
        const int pf = fmt ? fmt[i] : WZ_FMT_RGB24;
        const char* what = entries ? "frame-table entry" : "frame";
        WZCHK(frame_refusal(e, what, i, ptr[i], w[i], h[i], pf, -1, FC_PTR | FC_LIMIT));
        const uint64_t bytes = entries ? e->bound[entries[i]].bytes : wz_frame_bytes(w[i], h[i], pf);
        if (!bytes) return frame_refusal(e, what, i, ptr[i], w[i], h[i], pf, -1, FC_FMT);
        // pageable source: the runtime stages it (slow, synchronous); registered / pinned source: one DMA -- or no copy at all
        const uint8_t* dv = !(may_read && read_in_place(e, h[i])) ? nullptr : entries ? e->bound[entries[i]].dev : device_view(e, ptr[i], bytes);
        if (dv) {
            ptr[i] = dv;
            *in_place = true;
        } else {
            WZCHK(stage_frame(e, L, i, ptr[i], bytes, &ptr[i]));
        }
    }
    return WZ_OK;
}

extern "C" int wz_detect_batch(wz_engine_t* e, int n, const uint8_t* const* rgb, const int* w, const int* h,
                               const int* cam, wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    return wz_detect_batch_fmt(e, n, rgb, w, h, nullptr, cam, out, pass, ms);
}
extern "C" int wz_detect_batch_fmt(wz_engine_t* e, int n, const uint8_t* const* rgb, const int* w, const int* h, const int* fmt,
                                   const int* cam, wz_detection_t* const* out, uint8_t* const* pass, float* ms) {
    if (!e || !rgb || !w || !h) return wz_set_error(WZ_EINVAL, "wz_detect_batch: null argument");
    WZCHK(batch_refusal(e, 0, n, BC_N));
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipEventSynchronize(e->lanes[0].done));
    std::vector<const uint8_t*> dptr(rgb, rgb + n);
    bool in_place;
    WZCHK(place_frames(e, e->lanes[0], n, dptr.data(), w, h, fmt, nullptr, false, &in_place));   // (every frame staged, none read in place)
    WZCHK(wz_submit_device_fmt(e, 0, n, dptr.data(), w, h, fmt, cam));
    return collect_timed(e, n, out, pass, ms, t0);
}
// lane 0's rows handed over and the wall time since t0 into ms[n].  WZ_OK, or WZ_EINCOMPLETE: the rows are written (and timed), one
// frame's may be short
int collect_timed(wz_engine* e, int n, wz_detection_t* const* out, uint8_t* const* pass, float* ms, std::chrono::steady_clock::time_point t0) {
    const int rc = wz_collect(e, 0, out, pass);
    if (rc != WZ_OK && rc != WZ_EINCOMPLETE) return rc;
    const float el = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms)
        for (int i = 0; i < n; ++i) ms[i] = el;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// host frames, asynchronously: H2D of batch k+1 (DMA engine) under the kernels of batch k
// ------------------------------------------------------------------------------------------------
// Frame i of the batch going onto lane L: one copy into the lane's staging area, on the lane's stream.  From page-locked memory
// (wz_host_register) that is one SDMA transfer at PCIe rate; pageable memory is staged by the runtime.  (A copy KERNEL reading
// the frames through their device-mapped addresses -- one graph node per batch instead of one call per frame -- reaches
// 55 GB/s on its own, tools/micro/h2d_streams.hip, but only 23 GB/s beside the other lanes' kernels against the copies'
// 29 GB/s; a fifth stream for the copies alone, so that whole batches arrive back to back: 24.8 k against 31.5 k frames/s at
// 640x480 -- this stack runs four streams side by side, HISTORY.md part B: profiles/r03_host_path_*.)
// Where the device sees a page-locked host frame, or nullptr: inside a range wz_host_register locked (WzFrameDesc::rgb may then point
// at the frame itself and the resize kernel reads its tap rows over PCIe, no staging copy -- `host_read`).
const uint8_t* device_view(wz_engine* e, const uint8_t* host, uint64_t bytes) {
    for (const auto& r : e->host_ranges)
        if (host >= r.host && host + bytes <= r.host + r.bytes) return r.dev ? r.dev + (host - r.host) : nullptr;
    return nullptr;
}
// host_read policy for one frame: 1 = always in place, 2 = only when the vertical down-scale skips source rows (>= 2: at most half
// of the rows are tapped; below that nearly every row is, some twice, and one DMA of the whole frame moves fewer bytes)
bool read_in_place(const wz_engine* e, int h) {
    return e->host_read == 1 || (e->host_read == 2 && h >= 2 * (int)e->hdr.input_size);
}
// The LDS rule of the 10-bit formats.  e->pre_rows_lds is sized by the 8-bit formats (9 bytes a pixel of width: wz_preprocess_rows_lds, which
// sizes every launch and is left alone), one output row of a 10-bit frame needs 12 (wz_preprocess_rows_need).  A batch that holds a 10-bit
// frame whose row does not fit -- wider than 3405 pixels with the 40 KiB floor -- may not take the row-staged kernel: all of its frames are
// staged, none is read in place, and the batch takes the per-pixel kernel.  Every place that sets Lane::rows asks here first.
bool rows_fit(const wz_engine* e, int n, const int* w, const int* fmt) {
    for (int i = 0; fmt && i < n; ++i) {
        const int base = fmt[i] & WZ_FMT_BASE_MASK;
        if ((base == WZ_FMT_P010 || base == WZ_FMT_YUV420P10) && wz_preprocess_rows_need(w[i], fmt[i]) > (size_t)e->pre_rows_lds) return false;
    }
    return true;
}

int stage_frame(wz_engine* e, Lane& L, int i, const uint8_t* host, uint64_t bytes, const uint8_t** where) {
    uint8_t* dst = L.d_frames + e->frame_stride * i;
    HIPCHK(hipMemcpyAsync(dst, host, bytes, hipMemcpyHostToDevice, L.stream));
    *where = dst;
    return WZ_OK;
}
extern "C" int wz_submit_host(wz_engine_t* e, int slot, int n, const uint8_t* const* rgb, const int* w, const int* h,
                              const int* cam) {
    return wz_submit_host_fmt(e, slot, n, rgb, w, h, nullptr, cam);
}
extern "C" int wz_submit_host_fmt(wz_engine_t* e, int slot, int n, const uint8_t* const* rgb, const int* w, const int* h,
                                  const int* fmt, const int* cam) {
    if (!e || !rgb || !w || !h) return wz_set_error(WZ_EINVAL, "wz_submit_host: null argument");
    WZCHK(batch_refusal(e, slot, n));
    HIPCHK(hipSetDevice(e->device));
    Lane& L = e->lanes[slot];
    HIPCHK(hipEventSynchronize(L.done));   // the lane's previous batch (and its reads of the staging area) drained
    bool in_place;
    const bool fit = rows_fit(e, n, w, fmt);
    std::vector<const uint8_t*> dptr(rgb, rgb + n);
    WZCHK(place_frames(e, L, n, dptr.data(), w, h, fmt, nullptr, fit, &in_place));
    WZCHK(fill_desc(e, slot, n, dptr.data(), w, h, fmt, cam));
    L.rows = fit && (e->pre_rows || in_place);
    return run_batch(e, slot, n);
}

// Page-lock a host range (e.g. a FrameBuffer arena, watsor/stream/share.py:35-41) so that frames inside it go to
// the GPU by DMA at PCIe rate instead of through the runtime's bounce buffer.
extern "C" int wz_host_register(wz_engine_t* e, void* ptr, uint64_t bytes) {
    if (!e || !ptr || !bytes) return wz_set_error(WZ_EINVAL, "wz_host_register: bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipHostRegister(ptr, bytes, hipHostRegisterMapped));
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, ptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        dev = nullptr;                        // (not mapped on this platform: frames inside it are staged by DMA as before)
    }
    e->host_ranges.push_back({static_cast<const uint8_t*>(ptr), bytes, static_cast<const uint8_t*>(dev)});
    for (auto& f : e->bound)                  // (a frame table bound before its memory was page-locked)
        if (!f.dev) f.dev = device_view(e, f.host, f.bytes);
    return WZ_OK;
}
extern "C" int wz_host_unregister(wz_engine_t* e, void* ptr) {
    if (!e || !ptr) return wz_set_error(WZ_EINVAL, "wz_host_unregister: bad argument");
    HIPCHK(hipSetDevice(e->device));
    (void)sync_all(e);   // a copy (or a resize kernel reading in place) in flight may still be reading the range
    for (size_t k = 0; k < e->host_ranges.size(); ++k)
        if (e->host_ranges[k].host == ptr) {
            e->host_ranges.erase(e->host_ranges.begin() + k);
            break;
        }
    for (auto& f : e->bound)
        if (f.dev && f.host >= static_cast<const uint8_t*>(ptr)) f.dev = device_view(e, f.host, f.bytes);   // (re-resolved: stale views must not survive)
    HIPCHK(hipHostUnregister(ptr));
    return WZ_OK;
}

// ------------------------------------------------------------------------------------------------
// the worker's frame table: every Frame of every FrameBuffer described once (watsor/stream/share.py:27-41,76-81 -- sizes,
// pixels and rows of a frame never change after the buffers are created), a batch is then a list of indices
// (`frame_buffers[payload.sender].frames[payload.frame_index]`, watsor/detection/detector.py:104)
// ------------------------------------------------------------------------------------------------
extern "C" int wz_bind_frames(wz_engine_t* e, int n, const uint8_t* const* pixels, const int* w, const int* h, const int* fmt,
                              const int* cam, wz_detection_t* const* rows) {
    if (!e || n < 0 || (n && (!pixels || !w || !h || !rows))) return wz_set_error(WZ_EINVAL, "wz_bind_frames: bad argument");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));   // no batch in flight refers to the old table
    std::vector<wz_engine::BoundFrame> tbl((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int pf = fmt ? fmt[i] : WZ_FMT_RGB24;
        const int c = cam ? cam[i] : -1;
        WZCHK(frame_refusal(e, "frame-table entry", i, rows[i] ? pixels[i] : nullptr, w[i], h[i], pf, c, FC_PTR | FC_FMT | FC_LIMIT | FC_CAM_ID));
        const uint64_t bytes = wz_frame_bytes(w[i], h[i], pf);
        tbl[i] = {pixels[i], device_view(e, pixels[i], bytes), w[i], h[i], pf, c < 0 ? -1 : c, bytes, rows[i]};
    }
    for (int li = 0; li < e->n_lanes; ++li) e->lanes[li].bound_idx.clear();
    e->bound.swap(tbl);
    e->bound_tiles.clear();   // (the table is replaced: so is every tiled description of its entries)
    return WZ_OK;
}

extern "C" int wz_submit_bound(wz_engine_t* e, int slot, int n, const int32_t* entries) {
    if (!e || !entries) return wz_set_error(WZ_EINVAL, "wz_submit_bound: null argument");
    WZCHK(batch_refusal(e, slot, n));
    for (int i = 0; i < n; ++i)
        if (entries[i] < 0 || (size_t)entries[i] >= e->bound.size())
            return wz_set_error(WZ_EINVAL, "frame-table entry %d out of range [0,%zu)", entries[i], e->bound.size());
    if (!e->bound_tiles.empty())           // some entry of the table has a tiled description (wz_bind_tiles): does one of these?
        for (int i = 0; i < n; ++i)
            if (e->bound_tiles[entries[i]].kind != wz_engine::BOUND_PLAIN) return submit_bound_tiles(e, slot, n, entries);
    WZCHK(bound_drain(e, slot));
    Lane& L = e->lanes[slot];
    bool in_place;
    BoundBatch b;
    bound_gather(e, n, entries, b);
    const bool fit = rows_fit(e, n, b.w, b.fmt);
    WZCHK(place_frames(e, L, n, b.ptr.data(), b.w, b.h, b.fmt, entries, fit, &in_place));
#ifdef WZ_DEV_BUILD   // (wz_debug_bound_source: which leg each frame of this batch took)
    L.bound_src.resize(n);
    for (int i = 0; i < n; ++i) L.bound_src[i] = b.ptr[i] == e->bound[entries[i]].dev && b.ptr[i] != nullptr;
#endif
    // (the filter of a frame's camera may have been set for another size since the table was built: fill_desc checks)
    WZCHK(fill_desc(e, slot, n, b.ptr.data(), b.w, b.h, b.fmt, b.cam));
    L.rows = fit && (e->pre_rows || in_place);
    WZCHK(run_batch(e, slot, n));
    L.bound_idx.assign(entries, entries + n);
    return WZ_OK;
}

extern "C" int wz_collect_bound(wz_engine_t* e, int slot) {
    WZCHK(wz_wait(e, slot));
    Lane& L = e->lanes[slot];
    const LaneResult r = lane_result(L);
    if (L.bound_idx.empty() || (int)L.bound_idx.size() != r.n) return wz_set_error(WZ_EINVAL, "wz_collect_bound: lane %d holds no bound batch", slot);
    for (int i = 0; i < r.n; ++i)
        memcpy(e->bound[L.bound_idx[i]].rows, r.rows + (size_t)i * WZ_MAX_DETECTIONS, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS);
    L.bound_idx.clear();
    return lane_status(e, slot);
}

// ------------------------------------------------------------------------------------------------
// filters
// ------------------------------------------------------------------------------------------------
extern "C" int wz_set_camera_filter(wz_engine_t* e, int cam, int width, int height, const double* conf_thr,
                                    const double* area_thr, int n_zones, const uint8_t* zone_allow,
                                    const uint8_t* zone_fill) {
    if (!e || !conf_thr || !area_thr || width < 1 || height < 1) return wz_set_error(WZ_EINVAL, "wz_set_camera_filter: bad argument");
    if (cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_ELIMIT, "camera id %d out of range [0,%d)", cam, WZ_MAX_CAMS);
    if (n_zones < 0 || n_zones > WZ_MAX_ZONES_PER_CAM) return wz_set_error(WZ_ELIMIT, "%d zones > %d", n_zones, WZ_MAX_ZONES_PER_CAM);
    if (n_zones > 0 && !zone_fill) return wz_set_error(WZ_EINVAL, "zone_fill is null");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    // the new state is built aside and committed only when all of it exists: a failure (e.g. no memory for the
    // summed-area tables of a 1080p multi-zone mask) leaves the camera's previous filter intact
    WzCamFilter c;
    memset(&c, 0, sizeof(c));
    c.enabled = 1 | ((n_zones == 0 && zone_fill) ? 4 : 0);   // bit 2: a mask is configured but has no zone -> every row fails it
    c.width = width;
    c.height = height;
    c.n_zones = n_zones;
    memcpy(c.conf_thr, conf_thr, sizeof(double) * WZ_NUM_LABELS);
    memcpy(c.area_thr, area_thr, sizeof(double) * WZ_NUM_LABELS);
    for (int l = 0; l < WZ_NUM_LABELS; ++l)
        for (int z = 0; z < n_zones; ++z) c.allow[l][z] = zone_allow ? (zone_allow[(size_t)l * n_zones + z] ? 1 : 0) : 1;
    auto kept = [&](hipError_t err) { return wz_set_error(WZ_EHIP, "wz_set_camera_filter: %s (camera %d keeps its previous filter)", hipGetErrorString(err), cam); };
    DevBlock<int32_t> sat;
    if (n_zones > 0) {
        const size_t plane = (size_t)(width + 1) * (height + 1), fill = (size_t)width * height * n_zones;
        DevBlock<uint8_t> d_fill;
        hipError_t err = sat.alloc(plane * n_zones);
        if (err == hipSuccess) err = d_fill.alloc(fill);
        if (err == hipSuccess) err = lane0_copy(e, d_fill, zone_fill, fill, hipMemcpyHostToDevice);
        if (err == hipSuccess) {
            wz_launch_sat(d_fill, sat, width, height, n_zones, e->stream);
            err = hipStreamSynchronize(e->stream);
        }
        if (err != hipSuccess) return kept(err);
        c.sat = sat;
    }
    const hipError_t err = lane0_copy(e, e->d_cams + cam, &c, sizeof(WzCamFilter), hipMemcpyHostToDevice);
    if (err != hipSuccess) return kept(err);
    e->cam_sat[cam] = std::move(sat);   // (the old tables leave with `sat`; nothing in flight reads them: every lane was synchronised above)
    e->h_cams[cam] = c;
    return WZ_OK;
}

extern "C" int wz_set_camera_drop(wz_engine_t* e, int cam, int drop) {
    if (!e || cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_EINVAL, "wz_set_camera_drop: bad argument");
    if (!(e->h_cams[cam].enabled & 1)) return wz_set_error(WZ_EINVAL, "camera %d has no filter (wz_set_camera_filter first)", cam);
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    e->h_cams[cam].enabled = (e->h_cams[cam].enabled & ~2) | (drop ? 2 : 0);
    HIPCHK(lane0_copy(e, e->d_cams + cam, &e->h_cams[cam], sizeof(WzCamFilter), hipMemcpyHostToDevice));
    return WZ_OK;
}

extern "C" int wz_clear_camera_filter(wz_engine_t* e, int cam) {
    if (!e || cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_EINVAL, "wz_clear_camera_filter: bad argument");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    memset(&e->h_cams[cam], 0, sizeof(WzCamFilter));
    HIPCHK(lane0_copy(e, e->d_cams + cam, &e->h_cams[cam], sizeof(WzCamFilter), hipMemcpyHostToDevice));
    e->cam_sat[cam] = DevBlock<int32_t>();
    return WZ_OK;
}

extern "C" int wz_filter_rows(wz_engine_t* e, int cam, wz_detection_t* rows, uint8_t* pass) {
    if (!e || !rows || !pass || cam < 0 || cam >= WZ_MAX_CAMS) return wz_set_error(WZ_EINVAL, "wz_filter_rows: bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMemcpyAsync(e->d_tmp_rows, rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyHostToDevice, e->stream));
    wz_launch_filter_rows(e->d_cams, cam, e->d_tmp_rows, e->d_tmp_pass, e->stream);
    HIPCHK(hipMemcpyAsync(rows, e->d_tmp_rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(pass, e->d_tmp_pass, WZ_MAX_DETECTIONS, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return WZ_OK;
}

// ------------------------------------------------------------------------------------------------
// introspection / profiling
// ------------------------------------------------------------------------------------------------
extern "C" int wz_input_size(wz_engine_t* e) { return e ? (int)e->hdr.input_size : 0; }
extern "C" int wz_precision(wz_engine_t* e) { return e ? (int)e->hdr.precision : 0; }
extern "C" int wz_num_anchors(wz_engine_t* e) { return e ? (int)e->hdr.num_anchors : 0; }
extern "C" int wz_num_classes(wz_engine_t* e) { return e ? (int)e->hdr.num_classes : 0; }
extern "C" int wz_hp_blocks(wz_engine_t* e) { return e ? (int)e->hdr.hp_blocks : 0; }
extern "C" double wz_nms_iou(wz_engine_t* e) { return e ? (double)e->hdr.iou_threshold : 0.0; }

#ifdef WZ_DEV_BUILD   // ---- everything below this line exists in libwatsor_hip_dev.so only (include/watsor_hip.h, last section)
extern "C" int wz_num_tensors(wz_engine_t* e) { return e ? (int)e->hdr.n_tensors : 0; }
extern "C" int wz_num_ops(wz_engine_t* e) { return e ? (int)e->hdr.n_ops : 0; }

extern "C" int wz_tensor_info(wz_engine_t* e, int idx, char* name, int namelen, int* h, int* w, int* c) {
    if (!e || idx < 0 || idx >= (int)e->hdr.n_tensors) return wz_set_error(WZ_EINVAL, "tensor index %d", idx);
    const WzTensorDesc& t = e->tensors[idx];
    if (name && namelen > 0) snprintf(name, namelen, "%s", t.name);
    if (h) *h = t.h;
    if (w) *w = t.w;
    if (c) *c = t.c;
    return WZ_OK;
}

extern "C" int wz_tensor_flags(wz_engine_t* e, int idx) {
    if (!e || idx < 0 || idx >= (int)e->hdr.n_tensors) return wz_set_error(WZ_EINVAL, "tensor index %d", idx);
    return e->tensors[idx].flags;
}


extern "C" int wz_op_info(wz_engine_t* e, int idx, char* name, int namelen, int* dims) {
    if (!e || idx < 0 || idx >= (int)e->hdr.n_ops) return wz_set_error(WZ_EINVAL, "op index %d", idx);
    const WzOpDesc& o = e->ops[idx];
    if (name && namelen > 0) snprintf(name, namelen, "%s", o.name);
    if (dims) {
        // WZ_OP_MBCONV: cin = block input channels, slot 11 = depthwise (expanded) channels
        // (a stem-fused block reports cin = 3, the image channels)
        const int v[12] = {o.kind, o.kind == WZ_OP_MBCONV ? (o.stem ? 3 : o.cin0 ? o.cin0 : o.cmid) : o.cin, o.cout, o.ksize, o.stride,
                           o.hin, o.win, o.hout, o.wout, o.n_pad, o.kc, o.kind == WZ_OP_MBCONV ? o.cmid : 0};
        memcpy(dims, v, sizeof(v));
    }
    return WZ_OK;
}

extern "C" int wz_debug_nms(wz_engine_t* e, int n, uint64_t* out) {
    if (!e || !out || n < 1 || n > e->max_batch) return wz_set_error(WZ_EINVAL, "wz_debug_nms: bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out, e->lanes[0].post.dbg, (size_t)n * 16 * 8, hipMemcpyDeviceToHost));
    return WZ_OK;
}

extern "C" int wz_debug_post_lane(wz_engine_t* e, int slot, int n, float* box_enc, float* logits, float* boxes, float* scores,
                                  int32_t* classes, int32_t* num, uint64_t* dbg, int32_t* flags) {
    if (!e || slot < 0 || slot >= e->n_lanes || n < 1 || n > e->max_batch) return wz_set_error(WZ_EINVAL, "wz_debug_post_lane: bad argument");
    HIPCHK(hipSetDevice(e->device));
    const Lane& L = e->lanes[slot];
    HIPCHK(hipStreamSynchronize(L.stream));
    const size_t A = e->hdr.num_anchors, C = e->hdr.num_classes, T = e->hdr.max_total;
    if (T != WZ_MAX_DETECTIONS) return wz_set_error(WZ_EINVAL, "wz_debug_post_lane: max_total %zu, expected %d", T, WZ_MAX_DETECTIONS);
    if (box_enc) HIPCHK(hipMemcpy(box_enc, L.d_box_enc, n * A * 16, hipMemcpyDeviceToHost));
    if (logits) HIPCHK(hipMemcpy(logits, L.d_logits, n * A * C * 4, hipMemcpyDeviceToHost));
    if (boxes) HIPCHK(hipMemcpy(boxes, L.post.det_boxes, n * T * 16, hipMemcpyDeviceToHost));
    if (scores) HIPCHK(hipMemcpy(scores, L.post.det_scores, n * T * 4, hipMemcpyDeviceToHost));
    if (classes) HIPCHK(hipMemcpy(classes, L.post.det_classes, n * T * 4, hipMemcpyDeviceToHost));
    if (num) HIPCHK(hipMemcpy(num, L.post.det_num, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (dbg) HIPCHK(hipMemcpy(dbg, L.post.dbg, (size_t)n * 16 * 8, hipMemcpyDeviceToHost));
    if (flags) {   // of the batch last run: the launches of its graph key, whether they were issued one by one or replayed
        const auto it = L.forms.find(L.key);   // (no batch yet, only stage-level calls: 0, 0)
        flags[0] = it == L.forms.end() ? 0 : it->second.post_mode & 1;
        flags[1] = it == L.forms.end() ? 0 : (it->second.post_mode >> 1) & 1;
    }
    return WZ_OK;
}

extern "C" int wz_debug_mbconv(wz_engine_t* e, uint64_t* out, int32_t* groups) {
    if (!e || !out || !e->d_mbdbg) return wz_set_error(WZ_EINVAL, "wz_debug_mbconv: create the engine with WZ_MB_DEBUG=1");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    HIPCHK(hipMemcpy(out, e->d_mbdbg, (size_t)e->hdr.n_ops * 16 * 8, hipMemcpyDeviceToHost));
    if (groups) memcpy(groups, e->mb_groups.data(), sizeof(int) * e->hdr.n_ops);
    return WZ_OK;
}

// ---- lane stamps (`make stamps`; tools/lane_overlap.py): entry / exit of every launch of the batch last run on `slot`, 100 MHz ticks
extern "C" int wz_debug_lane_stamps(wz_engine_t* e, int slot, uint64_t* out, int cap) {
#if WZ_LANE_STAMPS
    if (!e || !out || slot < 0 || slot >= e->n_lanes) return wz_set_error(WZ_EINVAL, "wz_debug_lane_stamps: bad argument");
    const Lane& L = e->lanes[slot];
    const int k = L.post.stamps_n;          // launches in front of the NMS kernel; its own pairs (one per frame) follow and are folded here
    if (!L.hstamps.h || k <= 0 || cap < k + 1) return wz_set_error(WZ_EINVAL, "wz_debug_lane_stamps: no stamped batch on lane %d (or cap %d < %d)", slot, cap, k + 1);
    for (int i = 0; i < 2 * k; ++i) out[i] = L.hstamps.h[i];
    uint64_t t0 = ~0ull, t1 = 0;
    for (int f = 0; f < L.n; ++f) {
        t0 = std::min<uint64_t>(t0, L.hstamps.h[2 * (k + f)]);
        t1 = std::max<uint64_t>(t1, L.hstamps.h[2 * (k + f) + 1]);
    }
    out[2 * k] = t0;
    out[2 * k + 1] = t1;
    return k + 1;
#else
    (void)e; (void)slot; (void)out; (void)cap;
    return wz_set_error(WZ_EINVAL, "wz_debug_lane_stamps: this library was not built with -DWZ_LANE_STAMPS=1 (`make stamps`)");
#endif
}
// launch `idx` of that batch: kernel name, dims = {workgroups, threads per workgroup, LDS bytes (static + dynamic), workgroups a CU holds}
extern "C" int wz_debug_lane_launch(wz_engine_t* e, int slot, int idx, char* name, int namelen, int* dims) {
#if WZ_LANE_STAMPS
    if (!e || slot < 0 || slot >= e->n_lanes || !dims) return wz_set_error(WZ_EINVAL, "wz_debug_lane_launch: bad argument");
    Lane& L = e->lanes[slot];
    const auto it = L.forms.find(L.key);
    if (it == L.forms.end() || idx < 0 || idx >= (int)it->second.notes.size()) return wz_set_error(WZ_EINVAL, "wz_debug_lane_launch: no launch %d", idx);
    const WzLaunchNote& ln = it->second.notes[idx];
    HIPCHK(hipSetDevice(e->device));
    const char* nm = hipKernelNameRefByPtr(ln.func, L.stream);
    if (name && namelen > 0) snprintf(name, namelen, "%s", nm ? nm : "?");
    hipFuncAttributes fa;
    memset(&fa, 0, sizeof(fa));
    (void)hipFuncGetAttributes(&fa, ln.func);
    const int threads = (int)(ln.block[0] * ln.block[1] * ln.block[2]);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, ln.func, threads, ln.lds) != hipSuccess) { (void)hipGetLastError(); per_cu = 0; }
    dims[0] = (int)(ln.grid[0] * ln.grid[1] * ln.grid[2]);
    dims[1] = threads;
    dims[2] = (int)fa.sharedSizeBytes + (int)ln.lds;
    dims[3] = per_cu;
    dims[4] = fa.numRegs;
    return (int)it->second.notes.size();
#else
    (void)e; (void)slot; (void)idx; (void)name; (void)namelen; (void)dims;
    return wz_set_error(WZ_EINVAL, "wz_debug_lane_launch: this library was not built with -DWZ_LANE_STAMPS=1 (`make stamps`)");
#endif
}

extern "C" int wz_num_stages(wz_engine_t* e) { return e ? (int)e->stage_names.size() : 0; }
extern "C" int wz_stage_name(wz_engine_t* e, int stage, char* name, int namelen) {
    if (!e || stage < 0 || stage >= (int)e->stage_names.size()) return wz_set_error(WZ_EINVAL, "stage index %d", stage);
    snprintf(name, namelen, "%s", e->stage_names[stage].c_str());
    return WZ_OK;
}

extern "C" int wz_profile_device(wz_engine_t* e, int n, const uint8_t* const* d_rgb, const int* w, const int* h,
                                 int reps, float* stage_ms) {
    return wz_profile_stages(e, n, d_rgb, w, h, reps, 1, stage_ms);
}

extern "C" int wz_profile_stages(wz_engine_t* e, int n, const uint8_t* const* d_rgb, const int* w, const int* h,
                                 int reps, int inner, float* stage_ms) {
    if (!e || !stage_ms || reps < 1 || inner < 1 || inner > 64) return wz_set_error(WZ_EINVAL, "wz_profile_stages: bad argument");
    HIPCHK(hipSetDevice(e->device));
    WZCHK(sync_all(e));
    WZCHK(fill_desc(e, 0, n, d_rgb, w, h, nullptr, nullptr));
    e->lanes[0].rows = e->pre_rows;
    const size_t ns = e->stage_names.size();
    std::vector<double> acc(ns, 0.0);
    StageTimer t;
    t.s = e->stream;
    for (int r = 0; r < reps + 1; ++r) {   // first repetition is an untimed warm-up
        t.used = 0;
        t.mark();
        enqueue_batch(e, e->lanes[0], e->lanes[0].forms[n | (e->lanes[0].rows ? 1 << 16 : 0)], n, &t, inner);
        HIPCHK(hipStreamSynchronize(e->stream));
        if (t.used != ns + 1) return wz_set_error(WZ_EINVAL, "profile: %zu marks for %zu stages", t.used, ns);
        if (r == 0) continue;
        for (size_t i = 0; i < ns; ++i) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, t.ev[i], t.ev[i + 1]));
            acc[i] += ms;
        }
    }
    for (size_t i = 0; i < ns; ++i) stage_ms[i] = (float)(acc[i] / reps);
    for (hipEvent_t ev : t.ev) (void)hipEventDestroy(ev);
    return WZ_OK;
}

#endif   // WZ_DEV_BUILD

// ------------------------------------------------------------------------------------------------
// device memory helpers
// ------------------------------------------------------------------------------------------------
extern "C" int wz_dev_alloc(wz_engine_t* e, uint64_t bytes, void** d_ptr) {
    if (!e || !d_ptr) return wz_set_error(WZ_EINVAL, "wz_dev_alloc: null argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipMalloc(d_ptr, bytes));
    return WZ_OK;
}
extern "C" int wz_dev_free(wz_engine_t* e, void* d_ptr) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_dev_free: null engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipFree(d_ptr));
    return WZ_OK;
}
extern "C" int wz_dev_upload(wz_engine_t* e, void* d_dst, const void* h_src, uint64_t bytes) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_dev_upload: null engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(lane0_copy(e, d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return WZ_OK;
}
extern "C" int wz_dev_download(wz_engine_t* e, void* h_dst, const void* d_src, uint64_t bytes) {
    if (!e) return wz_set_error(WZ_EINVAL, "wz_dev_download: null engine");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(lane0_copy(e, h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return WZ_OK;
}

#ifdef WZ_DEV_BUILD
// ------------------------------------------------------------------------------------------------
// stage-level entry points (parity tests)
// ------------------------------------------------------------------------------------------------
extern "C" int wz_stage_preprocess(wz_engine_t* e, const uint8_t* rgb, int w, int h, uint16_t* out_half) {
    return wz_stage_preprocess_fmt(e, rgb, w, h, WZ_FMT_RGB24, out_half);
}
extern "C" int wz_stage_preprocess_fmt(wz_engine_t* e, const uint8_t* rgb, int w, int h, int fmt, uint16_t* out_half) {
    if (!e || !rgb || !out_half) return wz_set_error(WZ_EINVAL, "wz_stage_preprocess: null argument");
    if (w > e->max_w || h > e->max_h || (size_t)w * h * 3 > e->frame_stride) return wz_set_error(WZ_ELIMIT, "frame too large");
    const uint64_t bytes = wz_frame_bytes(w, h, fmt);
    if (!bytes) return wz_set_error(WZ_EINVAL, "pixel format 0x%x at %dx%d: %s", fmt, w, h, fmt_refusal(w, h, fmt));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(e->lanes[0].d_frames, rgb, bytes, hipMemcpyHostToDevice));   // (lane 0's staging area: its stream was drained above)
    const uint8_t* p = e->lanes[0].d_frames;
    WZCHK(fill_desc(e, 0, 1, &p, &w, &h, &fmt, nullptr));
    HIPCHK(hipMemcpyAsync(e->lanes[0].d_desc, e->lanes[0].desc.h, sizeof(WzFrameDesc), hipMemcpyHostToDevice, e->stream));
    const int S = (int)e->hdr.input_size;
    wz_launch_preprocess(e->lanes[0].d_desc, 1, S, e->lanes[0].tptr[input_tensor_index(e)], e->stream, input_is_pair(e), nullptr,
                         e->hdr.resize_mode == 1, nullptr, e->pre_rows && rows_fit(e, 1, &w, &fmt) ? e->pre_rows_lds : 0);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(out_half, e->lanes[0].tptr[input_tensor_index(e)], tensor_frame_bytes(e, input_tensor_index(e)),
                     hipMemcpyDeviceToHost));
    return WZ_OK;
}

extern "C" int wz_stage_forward(wz_engine_t* e, int n, const uint16_t* in_half, float* box_enc, float* logits) {
    if (!e || !in_half) return wz_set_error(WZ_EINVAL, "wz_stage_forward: null argument");
    WZCHK(batch_refusal(e, 0, n, BC_N));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int S = (int)e->hdr.input_size;
    if (input_is_pair(e)) {   // the given halves are the "hi" parts, the "lo" parts are zero (the input is exactly these halves)
        std::vector<uint16_t> pair((size_t)n * S * S * 8, 0);
        for (size_t px = 0; px < (size_t)n * S * S; ++px) memcpy(&pair[px * 8], in_half + px * 4, 8);
        HIPCHK(hipMemcpy(e->lanes[0].tptr[input_tensor_index(e)], pair.data(), pair.size() * 2, hipMemcpyHostToDevice));
    } else {
        HIPCHK(hipMemcpy(e->lanes[0].tptr[input_tensor_index(e)], in_half, (size_t)n * S * S * 4 * 2, hipMemcpyHostToDevice));
    }
    enqueue_network(e, e->lanes[0], n, nullptr, false);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    if (box_enc) HIPCHK(hipMemcpy(box_enc, e->lanes[0].d_box_enc, (size_t)n * e->hdr.num_anchors * 16, hipMemcpyDeviceToHost));
    if (logits)
        HIPCHK(hipMemcpy(logits, e->lanes[0].d_logits, (size_t)n * e->hdr.num_anchors * e->hdr.num_classes * 4, hipMemcpyDeviceToHost));
    return WZ_OK;
}

extern "C" int wz_stage_block_at(wz_engine_t* e, int op, int n, const void* d_in, int launch_frames) {
    if (!e || !d_in || op < 0 || op >= (int)e->hdr.n_ops || launch_frames < 0) return wz_set_error(WZ_EINVAL, "wz_stage_block_at: bad argument");
    WZCHK(batch_refusal(e, 0, n, BC_N));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (enqueue_block_at(e, e->lanes[0], n, (uint32_t)op, d_in, launch_frames) != 0) return wz_set_error(WZ_EINVAL, "wz_stage_block_at: op %d is not a fused block with a kernel", op);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    return WZ_OK;
}

extern "C" int wz_stage_read_tensor(wz_engine_t* e, int idx, int frame, uint16_t* out_half) {
    if (!e || !out_half || idx < 0 || idx >= (int)e->hdr.n_tensors || frame < 0 || frame >= e->max_batch)
        return wz_set_error(WZ_EINVAL, "wz_stage_read_tensor: bad argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t per = tensor_frame_bytes(e, idx);   // a pair tensor: 2c halves per pixel, hi then lo
    HIPCHK(hipMemcpy(out_half, (const uint8_t*)e->lanes[0].tptr[idx] + per * frame, per, hipMemcpyDeviceToHost));
    return WZ_OK;
}

extern "C" int wz_stage_postprocess(wz_engine_t* e, int n, const float* box_enc, const float* logits, float* boxes,
                                    float* scores, int32_t* classes, int32_t* num) {
    if (!e || !box_enc || !logits) return wz_set_error(WZ_EINVAL, "wz_stage_postprocess: null argument");
    WZCHK(batch_refusal(e, 0, n, BC_N));
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t A = e->hdr.num_anchors, C = e->hdr.num_classes, T = e->hdr.max_total;
    HIPCHK(hipMemcpy(e->lanes[0].d_box_enc, box_enc, n * A * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->lanes[0].d_logits, logits, n * A * C * 4, hipMemcpyHostToDevice));
    enqueue_post(e, e->lanes[0], false, n, nullptr);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    if (boxes) HIPCHK(hipMemcpy(boxes, e->lanes[0].post.det_boxes, n * T * 16, hipMemcpyDeviceToHost));
    if (scores) HIPCHK(hipMemcpy(scores, e->lanes[0].post.det_scores, n * T * 4, hipMemcpyDeviceToHost));
    if (classes) HIPCHK(hipMemcpy(classes, e->lanes[0].post.det_classes, n * T * 4, hipMemcpyDeviceToHost));
    if (num) HIPCHK(hipMemcpy(num, e->lanes[0].post.det_num, n * 4, hipMemcpyDeviceToHost));
    return WZ_OK;
}

// The post-processing a real batch runs, on caller-provided head outputs: everything behind the head convolutions, by the launches
// of enqueue_batch.  The given values go in as the single K slice of every head's partial sums (zero bias: 0 + x + 0 is x, bit for
// bit), the grouped reduce finishes them -- stores them, decodes the boxes, marks the candidates against lane 0's hint_logit -- and
// the NMS kernel reads its first band from the bit map and writes the rows.
extern "C" int wz_stage_post_production(wz_engine_t* e, int n, const float* box_enc, const float* logits, int w, int h,
                                        wz_detection_t* rows) {
    if (!e || !box_enc || !logits || !rows) return wz_set_error(WZ_EINVAL, "wz_stage_post_production: null argument");
    WZCHK(batch_refusal(e, 0, n, BC_N));
    if (e->hdr.max_total != WZ_MAX_DETECTIONS) return wz_set_error(WZ_EINVAL, "wz_stage_post_production: max_total %d, expected %d", (int)e->hdr.max_total, WZ_MAX_DETECTIONS);
    HIPCHK(hipSetDevice(e->device));
    Lane& L = e->lanes[0];
    HIPCHK(hipStreamSynchronize(L.stream));
    const size_t A = e->hdr.num_anchors, C = e->hdr.num_classes;
    WzReduceGroup g;
    memset(&g, 0, sizeof(g));
    std::vector<float> host;
    std::vector<size_t> offs;
    size_t covered = 0;
    for (int i = 0; i < (int)e->hdr.n_ops; ++i) {
        const WzOpDesc& op = e->ops[i];
        if (op.out_mode == WZ_OUT_ACT) continue;
        const int apl = op.anchors_per_loc, hw = op.hout * op.wout;
        if (op.out_mode != WZ_OUT_HEAD || g.n >= WZ_REDUCE_GROUP_MAX || op.n_box != apl * 4 || op.cout != apl * (4 + (int)C) ||
            op.n_pad < op.cout || (size_t)op.n_pad * 4 > 4096 || (size_t)op.anchor_off + (size_t)hw * apl > A)
            return wz_set_error(WZ_EINVAL, "wz_stage_post_production: op %d (%s) is no [box | class] head this entry can feed", i, op.name);
        WzConvArgs a = conv_args(e, L, op, n);   // (the grouped reduce reads the epilogue's part of it)
        head_outputs(e, L, op, a);
        a.bias = reinterpret_cast<const float*>(e->d_zeros.p);   // 4 KiB of zeros: n_pad floats at most (checked above)
        a.splitk = 1;
        offs.push_back(host.size());
        host.resize(host.size() + (size_t)a.M * a.n_pad, 0.0f);
        float* part = host.data() + offs.back();
        for (int b = 0; b < n; ++b)
            for (int pix = 0; pix < hw; ++pix) {
                float* row = part + ((size_t)b * hw + pix) * a.n_pad;
                const size_t an0 = (size_t)b * A + op.anchor_off + (size_t)pix * apl;
                memcpy(row, box_enc + an0 * 4, sizeof(float) * apl * 4);
                memcpy(row + apl * 4, logits + an0 * C, sizeof(float) * apl * C);
            }
        wz_reduce_group_add(g, a, nullptr);
        covered += (size_t)hw * apl;
    }
    if (g.n == 0 || covered != A) return wz_set_error(WZ_EINVAL, "wz_stage_post_production: the heads cover %zu of %zu anchors", covered, A);
    DevBlock<float> d_part;
    HIPCHK(d_part.alloc(host.size()));
    if (hipMemcpy(d_part, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return wz_set_error(WZ_EHIP, "wz_stage_post_production: upload");
    for (int i = 0; i < g.n; ++i) g.ws[i] = d_part + offs[i];
    g.decode = 1;
    g.list = 1;
    g.cbits_words = (int)((A * C + 31) >> 5);
    g.hint_logit = L.post.hint_logit;
    g.cbits = L.post.cbits;
    g.pc = e->pc;
    g.anchors = L.post.anchors;
    g.boxes = L.post.boxes;
    g.valid = L.post.valid;
    for (int i = 0; i < n; ++i) {
        WzFrameDesc& d = L.desc.h[i];
        memset(&d, 0, sizeof(d));
        d.w = w;
        d.h = h;
        d.cam = -1;
    }
    if (hipMemcpyAsync(L.d_desc, L.desc.h, sizeof(WzFrameDesc) * n, hipMemcpyHostToDevice, L.stream) != hipSuccess) return wz_set_error(WZ_EHIP, "wz_stage_post_production: descriptors");
    wz_launch_splitk_reduce_group(g, L.stream);
    enqueue_post(e, L, true, n, nullptr, true, true);
    L.key = n;
    L.forms[L.key].post_mode = 3;   // (wz_debug_post_lane: these launches decoded in the reduce and listed the candidates)
    if (hipStreamSynchronize(L.stream) != hipSuccess || hipGetLastError() != hipSuccess) return wz_set_error(WZ_EHIP, "wz_stage_post_production: launch");
    memcpy(rows, L.hrows.h, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS * n);
    return WZ_OK;
}

extern "C" int wz_stage_rows(wz_engine_t* e, int w, int h, const float* boxes, const float* scores,
                             const int32_t* classes, wz_detection_t* rows) {
    if (!e || !boxes || !scores || !classes || !rows) return wz_set_error(WZ_EINVAL, "wz_stage_rows: null argument");
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const size_t T = e->hdr.max_total;
    HIPCHK(hipMemcpy(e->lanes[0].post.det_boxes, boxes, T * 16, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->lanes[0].post.det_scores, scores, T * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->lanes[0].post.det_classes, classes, T * 4, hipMemcpyHostToDevice));
    WzFrameDesc& d = e->lanes[0].desc.h[0];
    memset(&d, 0, sizeof(d));
    d.w = w;
    d.h = h;
    d.cam = -1;
    HIPCHK(hipMemcpyAsync(e->lanes[0].d_desc, e->lanes[0].desc.h, sizeof(WzFrameDesc), hipMemcpyHostToDevice, e->stream));
    wz_launch_rows(e->lanes[0].post, e->lanes[0].d_desc, e->d_cams, 1, e->pc.max_total, e->d_tmp_rows, e->d_tmp_pass, e->stream);
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipMemcpy(rows, e->d_tmp_rows, sizeof(wz_detection_t) * WZ_MAX_DETECTIONS, hipMemcpyDeviceToHost));
    return WZ_OK;
}
#endif   // WZ_DEV_BUILD

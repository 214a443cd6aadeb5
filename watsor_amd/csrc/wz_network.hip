// What a batch launches between the resize kernel and the post-processing: the engine's ops, one after the other, on the lane's stream
// (enqueue_network), and what can be known about them before the first batch (network_prepare, op_kernel_check).  Host code only.
//
// One place per decision: conv_args fills a WzConvArgs from an op, head_outputs routes the SSD heads' outputs, HeadPark holds the rule
// by which a head's partial sums wait at the top of the workspace for ONE reduce launch after the last op, and stage_slots says how
// many stage-timer brackets an op owns -- wz_create names the stages by it and the op loop below pads every op's marks up to it.
#include <string.h>

#include "wz_engine.h"

// lane stamps: the block of the next launch of the batch being enqueued (nullptr in every build but `make stamps`)
#if WZ_LANE_STAMPS
static unsigned long long* next_stamp(Lane& L) {
    if (!L.d_stamps || L.stamp_next > WZ_STAMP_SLOTS) return nullptr;
    return L.d_stamps + (size_t)(L.stamp_next++ - 1) * WZ_STAMP_WORDS;
}
#define WZ_STAMP_ARG(a) ((a).dbg = next_stamp(L))
#define WZ_STAMP_ARG2(a) ((a).dbg2 = next_stamp(L))
#define WZ_STAMP_GROUP(g) ((g).stamp = next_stamp(L))
#else
#define WZ_STAMP_ARG(a) ((void)0)
#define WZ_STAMP_ARG2(a) ((void)0)
#define WZ_STAMP_GROUP(g) ((void)0)
#endif

// ------------------------------------------------------------------------------------------------
// an op's launch arguments
// ------------------------------------------------------------------------------------------------
// one fused block (WZ_OP_MBCONV); `L` without tensors (load-time check, kernel attributes): the pointers stay null
static WzMbArgs mb_args(wz_engine* e, const Lane& L, const WzOpDesc& op) {
    const uint8_t* wbase = e->d_weights;
    WzMbArgs a;
    memset(&a, 0, sizeof(a));
    a.in = L.tptr.empty() ? nullptr : L.tptr[op.src];
    a.we = (op.cin0 > 0 || op.stem) ? (const half_t*)(wbase + op.we_off) : nullptr;
    a.be = (op.cin0 > 0 || op.stem) ? (const float*)(wbase + op.be_off) : nullptr;
    a.wd = (const half_t*)(wbase + op.wd_off);
    a.bd = (const float*)(wbase + op.bd_off);
    a.wp = (const half_t*)(wbase + op.w_off);
    a.bp = (const float*)(wbase + op.b_off);
    a.res = (op.res >= 0 && !L.tptr.empty()) ? L.tptr[op.res] : nullptr;
    a.out = L.tptr.empty() ? nullptr : L.tptr[op.dst];
    a.hin = op.hin; a.win = op.win; a.hout = op.hout; a.wout = op.wout;
    a.cin0 = op.cin0; a.kc0 = op.kc0; a.nmid_pad = op.nmid_pad;
    a.cmid = op.cmid; a.cmid_pad = op.cmid_pad; a.kc = op.kc;
    a.cout = op.cout; a.n_pad = op.n_pad;
    a.stride = op.stride; a.pad_t = op.pad_t; a.pad_l = op.pad_l;
    a.hp = (op.flags & WZ_OPF_HP) ? 1 : 0;
    a.hp_out = (op.flags & WZ_OPF_HP_OUT) ? 1 : (op.flags & WZ_OPF_DUP_OUT) ? 2 : 0;
    a.qenc = (op.flags & WZ_OPF_QENC) ? 1 : 0;
    a.out2 = (op.dst2 > 0 && !L.tptr.empty()) ? L.tptr[op.dst2 - 1] : nullptr;
    a.has_out2 = op.dst2 > 0 ? 1 : 0;
    if (a.hp) {
        a.we_lo = (const half_t*)(wbase + op.we_lo_off);
        a.wp_lo = (const half_t*)(wbase + op.w_lo_off);
    }
    a.stem = op.stem;
    if (op.stem) {
        const WzTensorDesc& in = e->tensors[op.src];
        a.sin_h = in.h; a.sin_w = in.w;
        a.spad_t = op.stem_pad >> 16; a.spad_l = op.stem_pad & 0xffff;
    }
    return a;
}

// one separable layer (WZ_OP_DWSEP); `L` without tensors (load-time check): the pointers stay null
static WzDwsepArgs dwsep_args(wz_engine* e, const Lane& L, const WzOpDesc& op, int n) {
    const uint8_t* wbase = e->d_weights;
    WzDwsepArgs a;
    memset(&a, 0, sizeof(a));
    a.in = L.tptr.empty() ? nullptr : L.tptr[op.src];
    a.out = L.tptr.empty() ? nullptr : L.tptr[op.dst];
    a.wd = (const half_t*)(wbase + op.wd_off);
    a.bd = (const float*)(wbase + op.bd_off);
    a.wp = (const half_t*)(wbase + op.w_off);
    a.bp = (const float*)(wbase + op.b_off);
    a.M = n * op.hout * op.wout;
    a.hin = op.hin; a.win = op.win; a.hout = op.hout; a.wout = op.wout;
    a.cin = op.cin; a.kc = op.kc; a.cout = op.cout; a.n_pad = op.n_pad;
    a.stride = op.stride; a.pad_t = op.pad_t; a.pad_l = op.pad_l;
    return a;
}

// one convolution (WZ_OP_CONV) -- the only place that fills a WzConvArgs from an op: shape, weights, bias, residual, K chunks, the
// channel slice it writes, the zeros block and the debug slots.  Where the result goes is head_outputs'; the K split (`splitk`, `ws`,
// `frag_ws`, `dup_k`) is the launch's.  `L` without tensors: the tensor pointers stay null.  (fp32 engine: kc / kchunks count
// 16-channel chunks.)
WzConvArgs conv_args(wz_engine* e, const Lane& L, const WzOpDesc& op, int n) {
    const uint8_t* wbase = e->d_weights;
    WzConvArgs a;
    memset(&a, 0, sizeof(a));
    a.in = L.tptr.empty() ? nullptr : L.tptr[op.src];
    a.w = (const half_t*)(wbase + op.w_off);
    a.bias = (const float*)(wbase + op.b_off);
    a.res = (op.res >= 0 && !L.tptr.empty()) ? L.tptr[op.res] : nullptr;
    a.M = n * op.hout * op.wout;
    a.hin = op.hin; a.win = op.win; a.cin = op.cin;
    a.hout = op.hout; a.wout = op.wout; a.cout = op.cout; a.n_pad = op.n_pad;
    a.ksize = op.ksize; a.stride = op.stride; a.pad_t = op.pad_t; a.pad_l = op.pad_l; a.kc = op.kc;
    a.act = op.act; a.out_mode = op.out_mode;
    a.kchunks = op.ksize * op.ksize * op.kc;
    if (op.out_mode == WZ_OUT_ACT && op.dst_c != 0) {   // a channel slice of the output tensor (load_blob checked it)
        a.out_cstride = op.dst_c;
        a.out_coff = op.dst_coff;
    }
    a.zeros = e->d_zeros;
    a.dbg = e->d_mbdbg ? e->d_mbdbg + (size_t)(&op - e->ops) * 16 : nullptr;
    return a;
}

// where a convolution's result goes: its tensor, or -- the SSD heads -- its anchors' part of the lane's box-encoding / class-logit buffers
void head_outputs(wz_engine* e, const Lane& L, const WzOpDesc& op, WzConvArgs& a) {
    const int64_t A = e->hdr.num_anchors, C = e->hdr.num_classes;
    if (op.out_mode == WZ_OUT_ACT) {
        a.out = L.tptr.empty() ? nullptr : L.tptr[op.dst];
    } else if (op.out_mode == WZ_OUT_CLS) {
        a.out = L.d_logits;
        a.out_batch_stride = A * C;
        a.out_off = (int64_t)op.anchor_off * C;
    } else {   // WZ_OUT_BOX; WZ_OUT_HEAD: box columns -> d_box_enc, class columns -> d_logits
        a.out = L.d_box_enc;
        a.out_batch_stride = A * 4;
        a.out_off = (int64_t)op.anchor_off * 4;
        if (op.out_mode == WZ_OUT_HEAD) {
            a.out2 = L.d_logits;
            a.out2_batch_stride = A * C;
            a.out2_off = (int64_t)op.anchor_off * C;
            a.n_box = op.n_box;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// before the first batch
// ------------------------------------------------------------------------------------------------
int stage_slots(const WzOpDesc& op) { return (op.kind == WZ_OP_CONV || op.kind == WZ_OP_MBCONV) ? 2 : 1; }

// The kernel a fused block or a separable layer will run on exists for its shape: asked of the launchers themselves (prepare = true,
// batch 1, nothing is launched), by the ladder enqueue_network dispatches with.  The format checks are load_blob's.
int op_kernel_check(wz_engine* e, const WzOpDesc& op, const char* path) {
    const unsigned i = (unsigned)(&op - e->ops);
    Lane none;
    if (op.kind == WZ_OP_DWSEP) {
        if (wz_launch_dwsep(dwsep_args(e, none, op, 1), nullptr, true) != 0)
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): no depthwise-separable kernel for this shape (cin %d, cout %d, n_pad %d, %dx%d "
                                "stride %d)", path, i, op.name, op.cin, op.cout, op.n_pad, op.hin, op.win, op.stride);
    } else if (op.kind != WZ_OP_MBCONV) {
        return WZ_OK;
    } else if (op.flags & WZ_OPF_HP) {
        if (wz_launch_mbconv_hp(mb_args(e, none, op), 1, nullptr, true) != 0)
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): no split-operand kernel for this shape", path, i, op.name);
    } else if (op.stem) {
        if (wz_launch_mbconv_wave(mb_args(e, none, op), 1, nullptr, true) < 0)
            return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): no stem-fused kernel for this shape", path, i, op.name);
    } else if (op.dst2 > 0 ? wz_launch_mbconv_cs(mb_args(e, none, op), 1, nullptr, true) != 0
                           : wz_launch_mbconv(mb_args(e, none, op), 1, nullptr, true) != 0) {
        return wz_set_error(WZ_EFORMAT, "%s: op %u (%s): no fused-block kernel for this shape", path, i, op.name);
    }
    return WZ_OK;
}

// wz_create, on the engine's device: the kernel attributes of the fused-block kernels, and what the op list alone says about an op
void network_prepare(wz_engine* e) {
    const uint32_t n_ops = e->hdr.n_ops;
    Lane none;
    for (uint32_t i = 0; i < n_ops; ++i) {
        const WzOpDesc& op = e->ops[i];
        if (op.kind != WZ_OP_MBCONV) continue;
        if (op.flags & WZ_OPF_HP) {
            (void)wz_launch_mbconv_hp(mb_args(e, none, op), e->max_batch, nullptr, true);
            continue;
        }
        if (!op.stem) (void)wz_launch_mbconv(mb_args(e, none, op), e->max_batch, nullptr, true);
        (void)wz_launch_mbconv_wave(mb_args(e, none, op), e->max_batch, nullptr, true);
        (void)wz_launch_mbconv_cs(mb_args(e, none, op), e->max_batch, nullptr, true);
    }
    e->op_facts.assign(n_ops, wz_engine::OpFacts{0, 0});
    for (uint32_t i = 0; i < n_ops; ++i) {
        const WzOpDesc& op = e->ops[i];
        if (op.kind != WZ_OP_CONV) continue;
        // a 1x1 whose whole output tensor only the convolution behind it reads: the extras pair's structural precondition
        if (op.out_mode == WZ_OUT_ACT && op.ksize == 1 && op.dst_c == 0 && i + 1 < n_ops) {
            const WzOpDesc& nx = e->ops[i + 1];
            bool only = nx.kind == WZ_OP_CONV && nx.src == op.dst && nx.out_mode == WZ_OUT_ACT && op.res < 0 && nx.res < 0 && nx.dst_c == 0;
            for (uint32_t j = 0; only && j < n_ops; ++j)
                if (j != i + 1 && (e->ops[j].src == op.dst || e->ops[j].res == op.dst)) only = false;
            e->op_facts[i].sole_next = only;
        }
        // Conv_1 behind a block that stores its output twice (the robust program): the GEMM kernel reads one copy for both weight halves
        for (uint32_t j = 0; j < i; ++j)
            if (e->ops[j].dst == op.src && (e->ops[j].flags & WZ_OPF_DUP_OUT)) e->op_facts[i].dup_k = 1;
    }
}

// ------------------------------------------------------------------------------------------------
// the heads' parked partial sums
// ------------------------------------------------------------------------------------------------
// The heads write only into the box / logit buffers that the post kernels read at the very end, so their partial sums can wait: each
// head's slab is parked at the top of the workspace and ONE launch reduces them all after the last op (six launches fewer per batch).
// Everything else uses the workspace below `ws_top`.  The heads' convolutions share launches as well: those with a long K loop run
// on the wide tile kernel (k_conv_wide.hip), the others on the tile kernel (`big`) or, the 3x3 ... 1x1 maps, on wz_k_conv_group (`small`).
struct HeadPark {
    size_t ws_top;
    WzReduceGroup heads;
    WzConvGroup wide, big, small;
    int wide_T;            // K steps per slice of the wide kernel (0: no head goes there)
    int box_ops, box_ops_grouped;   // ops that produce box encodings / how many of them went into `heads`
    int head_ops;                   // ops that write box encodings or class logits

    // The wide kernel's K slices are chosen together, for the whole launch (one round over the CUs, slices of equal length), before
    // the first head is enqueued.
    void start(wz_engine* e, const Lane& L, int n) {
        ws_top = e->ws_bytes;
        heads.n = wide.n = big.n = small.n = 0;
        heads.first[0] = wide.first[0] = big.first[0] = small.first[0] = 0;
        heads.decode = 0;
        wide_T = box_ops = box_ops_grouped = head_ops = 0;
        if (e->hdr.precision == 32 || !e->conv_wide || !e->use_splitk || !e->defer_heads) return;
        int tiles[WZ_CONV_GROUP_MAX], steps[WZ_CONV_GROUP_MAX], cnt = 0;
        long long tile_bytes[WZ_CONV_GROUP_MAX];
        for (uint32_t i = 0; i < e->hdr.n_ops && cnt < WZ_CONV_GROUP_MAX; ++i) {
            if (e->ops[i].kind != WZ_OP_CONV) continue;
            const WzConvArgs a = conv_args(e, L, e->ops[i], n);
            if (!wz_conv_wide_applies(a) || a.M < e->wide_min_m) continue;
            wz_conv_wide_shape(a, &tiles[cnt], &steps[cnt]);
            tile_bytes[cnt] = 128ll * 4 * (((a.cout + 15) & ~15) / (((a.cout + 15) / 16 + WZ_WIDE_TILES - 1) / WZ_WIDE_TILES));
            ++cnt;
        }
        // (K slices sized for HALF the chip when other lanes are there to use the rest: at batch 8 T = 27 -> 41 steps per slice, 179 -> ~120
        // workgroups of this one-wave-per-SIMD kernel, a third fewer fp32 partial tiles: 49.8 k -> 50.5 k frames/s, p50 +8 us)
        // (two workgroups of that kernel share a CU: twice the slots in the same part of the chip)
        if (cnt > 0) wide_T = e->wide_T > 0 ? e->wide_T : wz_choose_wide_T(tiles, steps, tile_bytes, cnt, (e->n_lanes > 1 ? e->wide_cus : e->num_cus) * 2);
    }
    void count(const WzOpDesc& op) {
        if (op.out_mode == WZ_OUT_HEAD || op.out_mode == WZ_OUT_BOX) ++box_ops;
        if (op.out_mode != WZ_OUT_ACT) ++head_ops;
    }
    // THE parking rule.  May this op park `bytes` of partial sums, and where: a head, while the grouped reduce has an entry left and
    // the slab (whole 256 bytes) leaves at least half of the workspace to the other ops -- then the slab is taken from the top.
    float* slab(const wz_engine* e, const Lane& L, const WzOpDesc& op, size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        if (!e->defer_heads || op.out_mode == WZ_OUT_ACT || heads.n >= WZ_REDUCE_GROUP_MAX || bytes + (e->ws_bytes >> 1) > ws_top) return nullptr;
        ws_top -= bytes;
        return reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(L.d_ws.p) + ws_top);
    }
    // ... and the reduce of what was parked there: `a` with its final outputs
    void reduce_later(const WzOpDesc& op, const WzConvArgs& a, const float* parked) {
        wz_reduce_group_add(heads, a, parked);
        if (op.out_mode == WZ_OUT_HEAD || op.out_mode == WZ_OUT_BOX) ++box_ops_grouped;
    }
    // after the last op: the grouped launches, in the stage timer's slots "heads#big_convs", "heads#small_convs" (and, the caller's
    // mark behind it, "heads#splitk_reduce")
    void flush(wz_engine* e, Lane& L, StageTimer* t, bool with_post) {
        hipStream_t s = L.stream;
        // every box encoding is finished by the grouped reduce: let it decode the boxes as well (one launch less)
        L.decode_fused = heads.n > 0 && box_ops > 0 && box_ops == box_ops_grouped && e->fuse_decode;
        // ... and list the class logits that can reach the NMS kernel's first band
        L.cands_listed = with_post && L.decode_fused && head_ops == heads.n;
        wide.stamp = big.stamp = small.stamp = heads.stamp = nullptr;   // (set per launch in the stamps build only)
        if (wide.n > 0) { WZ_STAMP_GROUP(wide); wz_launch_conv_wide_group(wide, s); }
        if (big.n > 0) { WZ_STAMP_GROUP(big); wz_launch_conv_rs_group(big, s); }
        if (t) t->mark();
        if (small.n > 0) { WZ_STAMP_GROUP(small); wz_launch_conv_group(small, s); }
        if (t) t->mark();
        if (L.decode_fused) {
            heads.decode = 1;
            heads.pc = e->pc;
            heads.anchors = L.post.anchors;
            heads.boxes = L.post.boxes;
            heads.valid = L.post.valid;
        }
        heads.list = L.cands_listed ? 1 : 0;
        if (L.cands_listed) {
            heads.hint_logit = L.post.hint_logit;
            heads.cbits = L.post.cbits;
            heads.cbits_words = (e->pc.num_anchors * e->pc.num_classes + 31) >> 5;
        }
        if (heads.n > 0) { WZ_STAMP_GROUP(heads); wz_launch_splitk_reduce_group(heads, s); }
    }
};

// ------------------------------------------------------------------------------------------------
// the op families.  Each enqueues ONE op's launches; it marks the stage timer only BETWEEN two launches of the op (the op loop
// closes the op's slots), so the first launch is booked on the op's first slot and a second one, if any, on its second.
// ------------------------------------------------------------------------------------------------
struct Net {   // the batch being enqueued
    wz_engine* e;
    Lane& L;
    int n;
    StageTimer* t;
    hipStream_t s;
    HeadPark park;   // (started by enqueue_network: nothing of it is zeroed per batch)
    int launch_frames = 0;   // WzMbArgs::launch_frames of the fused blocks (enqueue_block_at)
    Net(wz_engine* e_, Lane& L_, int n_, StageTimer* t_) : e(e_), L(L_), n(n_), t(t_), s(L_.stream) {}
    void mark() { if (t) t->mark(); }
};

// stem, depthwise, pooling, 7x7 stem: one launch, fp16 or fp32
static void enqueue_simple(Net& x, const WzOpDesc& op) {
    wz_engine* e = x.e;
    Lane& L = x.L;
    hipStream_t s = x.s;
    const int n = x.n;
    const bool f32 = e->hdr.precision == 32;
    const uint8_t* wbase = e->d_weights;
    const float* bias = (const float*)(wbase + op.b_off);
    const int cs = op.dst_c ? op.dst_c : op.cout;   // (Inception: the op writes its slice of the module tensor, or a tensor of its own)
    switch (op.kind) {
    case WZ_OP_STEM:
        if (f32)
            wz_launch_stem_f32(L.tptr[op.src], (const float*)(wbase + op.w_off), bias, (float*)L.tptr[op.dst], n, op.hin, op.win, op.hout,
                               op.wout, op.pad_t, op.pad_l, s, input_is_pair(e));
        else
            wz_launch_stem(L.tptr[op.src], (const float*)(wbase + op.w_off), bias, L.tptr[op.dst], n, op.hin, op.win, op.hout, op.wout,
                           op.pad_t, op.pad_l, s);
        break;
    case WZ_OP_DW:
        if (f32)
            wz_launch_dw_f32((const float*)L.tptr[op.src], (const float*)(wbase + op.w_off), bias, (float*)L.tptr[op.dst], n, op.hin, op.win,
                             op.cin, op.hout, op.wout, op.stride, op.pad_t, op.pad_l, op.act, s);
        else
            wz_launch_dw(L.tptr[op.src], (const half_t*)(wbase + op.w_off), bias, L.tptr[op.dst], n, op.hin, op.win, op.cin, op.hout, op.wout,
                         op.stride, op.pad_t, op.pad_l, op.act, s);
        break;
    case WZ_OP_POOL: {
        const bool is_max = !(op.flags & WZ_OPF_POOL_AVG);
        if (f32)
            wz_launch_pool3_f32((const float*)L.tptr[op.src], (float*)L.tptr[op.dst], n, op.hin, op.win, op.cin, op.hout, op.wout, op.stride,
                                op.pad_t, op.pad_l, is_max, cs, op.dst_coff, s);
        else
            wz_launch_pool3(L.tptr[op.src], L.tptr[op.dst], n, op.hin, op.win, op.cin, op.hout, op.wout, op.stride, op.pad_t, op.pad_l,
                            is_max, cs, op.dst_coff, s);
        break;
    }
    default:   // WZ_OP_STEM7
        if (f32)
            wz_launch_stem7_f32(L.tptr[op.src], (const float*)(wbase + op.w_off), bias, (float*)L.tptr[op.dst], n, op.hin, op.win, op.hout,
                                op.wout, op.pad_t, op.pad_l, cs, op.dst_coff, input_is_pair(e), s);
        else
            wz_launch_stem7(L.tptr[op.src], (const half_t*)(wbase + op.w_off), bias, L.tptr[op.dst], n, op.hin, op.win, op.hout, op.wout,
                            op.pad_t, op.pad_l, cs, op.dst_coff, s);
    }
}

static void enqueue_dwsep(Net& x, uint32_t i, const WzOpDesc& op) {   // (load_blob refused every shape wz_launch_dwsep does not cover)
    Lane& L = x.L;
    WzDwsepArgs a = dwsep_args(x.e, L, op, x.n);
    WZ_STAMP_ARG(a);
    if (wz_launch_dwsep(a, x.s, false) != 0) L.launch_failed = (int)i + 1;
}

static void enqueue_mbconv(Net& x, uint32_t i, const WzOpDesc& op) {
    wz_engine* e = x.e;
    Lane& L = x.L;
    hipStream_t s = x.s;
    const int n = x.n;
    WzMbArgs a = mb_args(e, L, op);
    a.M = n * op.hout * op.wout;
    a.lone = L.lone ? 1 : 0;
    a.launch_frames = x.launch_frames;
    a.ws =(e->use_splitk || a.hp) ? L.d_ws : nullptr;   // (split-K partials of the plain blocks; the two-launch split blocks' project fragments)
    a.ws_bytes = x.park.ws_top;
    a.dbg = e->d_mbdbg ? e->d_mbdbg + (size_t)i * 16 : nullptr;
    WZ_STAMP_ARG(a);
    if (a.hp && wz_mbconv_hp2_applies(a, n)) {
        // the 10x10 split blocks of the robust program: two GEMM-shaped launches (k_mbconv_hp2.hip); the stage timer books the second one
        // on the op's (otherwise empty) reduce slot
        WZ_STAMP_ARG2(a);
        int r2 = wz_launch_mbconv_hp2(a, n, s, false, 1);
        x.mark();
        if (r2 >= 0) r2 = wz_launch_mbconv_hp2(a, n, s, false, 2);
        if (r2 < 0) L.launch_failed = (int)i + 1;
        if (e->d_mbdbg) e->mb_groups[i] = 1;
        return;
    }
    int groups = a.hp ? wz_launch_mbconv_hp(a, n, s, false)   // split-operand blocks (the `-p 16` program's first 13)
                      : wz_launch_mbconv_wave(a, n, s, false);   // large maps: one wavefront per pixel tile
    if (a.hp && groups < 0) L.launch_failed = (int)i + 1;   // nothing was enqueued for a split-operand block: run_batch reports it
    if (groups == -2 && (e->use_splitk || a.has_out2)) groups = wz_launch_mbconv_cs(a, n, s, false);   // small maps: channels over waves
    if (a.has_out2 && groups < 0) L.launch_failed = (int)i + 1;   // only the chunk-split kernel stores a second output
    if (groups == -2) groups = wz_launch_mbconv(a, n, s, false);
    if (e->d_mbdbg) e->mb_groups[i] = groups;
    if (groups > 1) {   // sum the channel groups' partials in a fixed order, + bias, + residual, -> fp16
        x.mark();
        WzConvArgs r;
        memset(&r, 0, sizeof(r));
        r.bias = a.bp; r.res = a.res; r.out = a.out;
        r.M = a.M; r.hout = a.hout; r.wout = a.wout; r.cout = a.cout; r.n_pad = a.n_pad;
        r.act = WZ_ACT_NONE; r.out_mode = WZ_OUT_ACT; r.splitk = groups;
        WZ_STAMP_ARG(r);
        wz_launch_splitk_reduce(r, L.d_ws, s);
    }
}

// fp32 engine: a convolution and, behind it in the same launcher, its split-K reduce -- unless the op is a head whose partial sums park
static void enqueue_conv_f32(Net& x, const WzOpDesc& op) {
    wz_engine* e = x.e;
    Lane& L = x.L;
    WzConvArgs a = conv_args(e, L, op, x.n);
    head_outputs(e, L, op, a);
    x.park.count(op);
    int sk = !e->use_splitk ? 1 : wz_conv_f32_use_rs(a) ? wz_choose_splitk_rs_f32(a.M, a.n_pad, a.kchunks) : wz_choose_splitk(a.M, a.n_pad, a.kchunks / 2);
    float* const parked = sk > 1 ? x.park.slab(e, L, op, (size_t)sk * a.M * a.n_pad * 4) : nullptr;
    if (parked) {
        // the heads' outputs are fp32 in both engines and their epilogue is the same: the partial sums are
        // parked and reduced (+ decoded, + candidates marked) by the same grouped launch as in the fp16 engine
        a.splitk = sk;
        a.ws = parked;
        wz_launch_conv_f32(a, x.s, false);
        x.park.reduce_later(op, a, parked);
        return;
    }
    if (wz_conv_ws_f32_applies(a)) {   // the extras chain: K split across the waves of a workgroup, no reduce
        a.splitk = 1;
        wz_launch_conv_ws_f32(a, x.s);
        return;
    }
    while (sk > 1 && (size_t)sk * a.M * a.n_pad * 4 > x.park.ws_top) --sk;
    a.splitk = sk;
    a.ws = L.d_ws;
    wz_launch_conv_f32(a, x.s);
}

// Two convolutions of the extras chain in one launch (k_extras_pair.hip): a 1x1 whose output only the 3x3 stride-2 convolution behind it
// reads, on the 5x5 / 3x3 / 2x2 maps -- three launches and three boundaries less per batch (not for slice outputs: the pair kernel
// stores whole tensors).  True: ops i and i + 1 are enqueued.
static bool enqueue_extras_pair(Net& x, uint32_t i) {
    wz_engine* e = x.e;
    Lane& L = x.L;
    WzConvArgs pa = conv_args(e, L, e->ops[i], x.n), pb = conv_args(e, L, e->ops[i + 1], x.n);
    head_outputs(e, L, e->ops[i], pa);
    head_outputs(e, L, e->ops[i + 1], pb);
    pa.splitk = pb.splitk = 1;
    if (!wz_extras_pair_applies(pa, pb)) return false;
    WZ_STAMP_ARG(pa);
    wz_launch_extras_pair(pa, pb, x.n, x.s);
    return true;
}

// fp16 engine.  Returns the ops enqueued: 2 when the extras pair took the next one as well (the launch is booked on the first slot of both ops' four).
static int enqueue_conv_f16(Net& x, uint32_t i, const WzOpDesc& op) {
    wz_engine* e = x.e;
    Lane& L = x.L;
    hipStream_t s = x.s;
    HeadPark& hp = x.park;
    if (e->op_facts[i].sole_next && enqueue_extras_pair(x, i)) return 2;
    WzConvArgs a = conv_args(e, L, op, x.n);
    head_outputs(e, L, op, a);
    void* const final_out = a.out;
    hp.count(op);
    int sk = 1;
    if (e->use_splitk)
        sk = wz_conv_use_lds(a) ? wz_choose_splitk_lds(a.M, a.n_pad, a.kchunks) : wz_choose_splitk(a.M, a.n_pad, a.kchunks);
    float* parked = nullptr;
    bool to_wide = hp.wide_T > 0 && hp.wide.n < WZ_CONV_GROUP_MAX && wz_conv_wide_applies(a) && a.M >= e->wide_min_m;
    if (to_wide) {   // its partial sums always go through the grouped reduce, also with a single K slice
        const size_t m16 = ((size_t)a.M + 15) & ~(size_t)15;   // (the wide kernel's partials are whole 16-pixel fragments)
        const int wsk = ((a.kchunks >> 1) + hp.wide_T - 1) / hp.wide_T;
        parked = hp.slab(e, L, op, (size_t)wsk * m16 * a.n_pad * 4);
        if (parked) sk = wsk;
        else to_wide = false;
    }
    if (!parked && sk > 1) parked = hp.slab(e, L, op, (size_t)sk * a.M * a.n_pad * 4);
    if (parked) {
        a.frag_ws = to_wide ? 1 : 0;   // (only the wide kernel and the grouped reduce behind it know that order)
        a.splitk = sk;
        a.out = parked;
        if (to_wide) {
            wz_conv_wide_group_add(hp.wide, a);
        } else if (hp.small.n < WZ_CONV_GROUP_MAX && wz_conv_groupable(a)) {
            wz_conv_group_add(hp.small, a);   // launched with the other small heads after the last op
        } else if (!(wz_conv_rs_groupable(a) && wz_conv_rs_group_add(hp.big, a))) {   // (the heads on the tile kernel: one launch, too)
            WZ_STAMP_ARG(a);
            wz_launch_conv(a, s);
        }
        a.out = final_out;   // its own reduce slot stays empty
        hp.reduce_later(op, a, parked);
        return 1;
    }
    a.dup_k = e->op_facts[i].dup_k;
    if (wz_gemm_1x1_applies(a)) {   // one launch, all of K per wave: no K split, nothing to reduce
        a.splitk = 1;
        WZ_STAMP_ARG(a);
        wz_launch_gemm_1x1(a, s);
        return 1;
    }
    if ((sk > 1 || a.M < 128) && wz_conv_ws_applies(a)) {   // the K split happens inside the workgroups: nothing to reduce
        // (on the 2x2 and 1x1 maps also where one wave per tile would walk all of K alone)
        a.splitk = 1;
        WZ_STAMP_ARG(a);
        wz_launch_conv_ws(a, s);
        return 1;
    }
    while (sk > 1 && (size_t)sk * a.M * a.n_pad * 4 > hp.ws_top) --sk;
    a.splitk = sk;
    if (sk > 1) {
        a.out = L.d_ws;
        WZ_STAMP_ARG(a);
        wz_launch_conv(a, s);
        x.mark();
        a.out = final_out;
        WZ_STAMP_ARG(a);
        wz_launch_splitk_reduce(a, L.d_ws, s);
    } else {
        WZ_STAMP_ARG(a);
        wz_launch_conv(a, s);
    }
    return 1;
}

#ifdef WZ_DEV_BUILD
// One fused block of the network on its own, its source tensor read at `d_in` instead of where the engine keeps it (wz_stage_block_at:
// the caller decides what lies around the tensor; a residual that IS the source tensor is read there too).  Everything else -- weights,
// outputs, launch shapes -- as in the network.  launch_frames > 0: a split-operand block takes at most that many frames per launch.
int enqueue_block_at(wz_engine* e, Lane& L, int n, uint32_t i, const void* d_in, int launch_frames) {
    const WzOpDesc& op = e->ops[i];
    if (op.kind != WZ_OP_MBCONV) return -1;
    Net x(e, L, n, nullptr);
    x.park.start(e, L, n);
    x.launch_frames = launch_frames;
    half_t* const kept = L.tptr[op.src];
    L.tptr[op.src] = static_cast<half_t*>(const_cast<void*>(d_in));
    L.launch_failed = 0;
    enqueue_mbconv(x, i, op);
    L.tptr[op.src] = kept;
    return L.launch_failed ? -1 : 0;
}
#endif

// with_post: the post-processing chain follows in the same stream (it consumes -- and resets -- the candidate list)
void enqueue_network(wz_engine* e, Lane& L, int n, StageTimer* t, bool with_post) {
    Net x(e, L, n, t);
    x.park.start(e, L, n);
    const bool f32 = e->hdr.precision == 32;
    for (uint32_t i = 0; i < e->hdr.n_ops;) {
        const WzOpDesc& op = e->ops[i];
        const size_t marks0 = t ? t->used : 0;
        int ops = 1;
        switch (op.kind) {
        case WZ_OP_DWSEP: enqueue_dwsep(x, i, op); break;
        case WZ_OP_MBCONV: enqueue_mbconv(x, i, op); break;
        case WZ_OP_CONV:
            if (f32) enqueue_conv_f32(x, op);
            else ops = enqueue_conv_f16(x, i, op);
            break;
        default: enqueue_simple(x, op);
        }
        // the op's stage slots (a fused pair: both ops'): whatever it did not mark itself stays an empty bracket
        size_t slots = 0;
        for (int k = 0; k < ops; ++k) slots += stage_slots(e->ops[i + k]);
        while (t && t->used < marks0 + slots) t->mark();
        i += ops;
    }
    x.park.flush(e, L, t, with_post);
    x.mark();
}

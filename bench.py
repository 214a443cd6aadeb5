"""Throughput / latency / roofline bench of the MI355X detection hot path.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W

A *step* is one pass of the hot path (resize+normalise -> SSD-MobileNet-v2 -> decode -> NMS -> 100
Detection rows per frame, D2H of the rows included) over one batch of synthetic frames that are
already resident in HBM.  Workload at N=1 = BASELINE.json configs[1]: one synthetic 640x480 RGB
stream, batch = 8 frames, 1 x MI355X.  For N > 1 every rank is an independent replica with its own
camera (cameras are the shard; no data-path collective -- SURVEY.md 8e), value = frames of all ranks
/ max-over-ranks time, scaling "weak".  `--gpus N` without a launcher (WORLD_SIZE unset) starts the N
ranks itself, one process per device ordinal -- the reference's scheme (`watsor/detection/detector.py:34-50`).

The timed region is exactly K steps (barrier + device synchronise on both sides, max over ranks);
`value` / `ms_per_step` are taken from it.  `--rounds R` repeats the region R times and reports the
MEDIAN region, min / max beside it; `--rounds 0` repeats it >= 25 times, until 1 s of them (one
K = 20 region lasts ~4 ms: a single sample of it is noise).

`--dump-outputs DIR` writes the detection rows the last timed step handed back (rank 0; ROW_DTYPE's
fields, one float64 array [batch, 100, ...] each) as DIR/<field>.npy.  The inputs are seeded: two
runs with the same arguments see the same frames and weights.

Rank 0 prints ONE JSON line (contract in the task description) extended with
  "p50_ms"      : median latency of synchronous batch-8 steps, frames in HBM
and, with `--full` only (each part can be left out again with its --no-* option):
  "parity"      : the north star's criterion checked LIVE on the engine that was timed: max |score - oracle score|
                  over the detection rows of 8 of the benchmark's frames (bar: 1e-3)
  "roofline"    : dominant kernel of the step, timed live with HIP events on the engine's own stream
  "legs"        : the other BASELINE configs as per-GPU shares (frames/s + p50), host-frame and plugin paths
  "default_program_engine" / "plain_fp16_engine" / "fp32_engine": the same workload on the other programs
  "cpu_baseline": the oracle (CPU restatement of the reference's TF detector) on this host's cores
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_PEAK_TFLOPS = 2500.0    # dense fp16/bf16 MFMA
WIDTH, HEIGHT, BATCH = 640, 480, 8
SCORE_TOLERANCE = 1e-3       # BASELINE.json north_star: "box scores within 1e-3 of the CPU reference"
MIN_ROUNDS, MAX_ROUNDS, ROUNDS_BUDGET_S = 25, 400, 1.0
RING = 5                     # batches of distinct frames the timed loop cycles through (coprime with the 4 lanes)
PROFILE_INNER = 8            # launches per bracket in the stage profile (wz_profile_stages)
# The program the headline is timed on: the ROBUST `-p 16` program (all 17 blocks on split operands, float-form chunk buffer on the
# large maps, Conv_1 with split weights) -- the one `python -m watsor_amd.engine` builds for weights whose BatchNorm-folded channels are
# spread over more than 0.45 decades, i.e. for a TRAINED checkpoint (per-channel ranges of a folded MobileNet-v2 differ by orders of
# magnitude -- the reason per-tensor quantisation of this network needs cross-layer equalisation).  It holds the north star's 1e-3 at
# 0 / 1 / 1.5 / 2 decades of spread (tests/test_gpu_stress.py); the default program, faster, holds it only on weights whose channels live
# at one scale -- such as this benchmark's seeded random-init weights -- and is reported beside it (`default_program_engine`).
HEADLINE_PROGRAM = dict(robust=True)


# --------------------------------------------------------------------------------------------------
# roofline
# --------------------------------------------------------------------------------------------------
def kernel_class(op, hp):
    from watsor_amd import arch
    if op["kind"] == arch.OP_STEM:
        return "wz_k_stem"
    if op["kind"] == arch.OP_DW:
        return "wz_k_dw"
    if op["kind"] == arch.OP_MBCONV:
        return "wz_k_mbconv_hp" if hp else "wz_k_mbconv"
    return "wz_k_conv<%d>" % op["ksize"]


def algorithmic_cost(op, n):
    """(flops, bytes) of one launch per the per-layer rule of SURVEY.md 8(d): fp16, every tensor once.
    A fused inverted-residual block is priced as the layers it computes (expand, depthwise, project), i.e.
    the bytes a layer-by-layer fp16 execution moves -- also for the split-operand blocks, whose extra bytes
    (pair tensors, hi + lo weights) and 3x MFMA work are the price of the tolerance, not algorithmic work."""
    from watsor_amd import arch
    M = n * op["hout"] * op["wout"]
    if op["kind"] == arch.OP_MBCONV:
        Min, cin, cmid, cout = n * op["hin"] * op["win"], op["cin"], op["cmid"], op["cout"]
        fl, by = 0.0, 0.0
        if cin == 3:                                                 # stem conv folded in (3x3 s2 on the 4-channel input)
            fl += 2.0 * Min * 32 * 27
            by += 2.0 * (n * (2 * op["hin"]) * (2 * op["win"]) * 4 + Min * 32) + 27 * 32 * 4
        elif cin != cmid:                                            # 1x1 expand
            fl += 2.0 * Min * cin * cmid
            by += 2.0 * (Min * cin + cin * cmid + Min * cmid)
        fl += 2.0 * M * cmid * 9                                     # depthwise 3x3
        by += 2.0 * (Min * cmid + 9 * cmid + M * cmid)
        fl += 2.0 * M * cmid * cout                                  # 1x1 project
        by += 2.0 * (M * cmid + cmid * cout + M * cout)
        return fl, by
    if op["kind"] == arch.OP_DW:
        c = op["cin"]
        return 2.0 * M * c * 9, 2.0 * (n * op["hin"] * op["win"] * c + 9 * c + M * c)
    if op["kind"] == arch.OP_STEM:
        return 2.0 * M * 32 * 27, 2.0 * (n * op["hin"] * op["win"] * 4 + M * 32) + 27 * 32 * 4
    cin = op["cin"] // 2 if (op["name"].endswith("Conv_1") and op["cin"] == 640) else op["cin"]   # (split weights double K, not the layer)
    K = op["ksize"] ** 2 * cin
    N = op["cout"]
    out_bytes = 4.0 if op["name"].startswith("BoxPredictor") else 2.0     # head outputs are fp32
    return 2.0 * M * N * K, 2.0 * (n * op["hin"] * op["win"] * cin + K * N) + out_bytes * M * N


def fused_min_bytes(op, n, hp, hp_out):
    """What a fused block launch has to move, as laid out in HBM: block input + weights + output, once each
    (pair tensors 4 bytes per value, split weights twice, fp32 depthwise weights)."""
    cin, cmid, cout = op["cin"], op["cmid"], op["cout"]
    es_in = 4.0 if hp else 2.0
    es_out = 4.0 if hp_out else 2.0
    es_w = 4.0 if hp else 2.0
    inp = n * (2 * op["hin"]) * (2 * op["win"]) * 4 if cin == 3 else n * op["hin"] * op["win"] * cin
    wts = (27 * 32 if cin == 3 else (cin * cmid if cin != cmid else 0)) + cmid * cout
    return es_in * inp + es_w * wts + (4.0 if hp else 2.0) * 9 * cmid + es_out * n * op["hout"] * op["wout"] * cout


def empty_bracket_ms(stages):
    """Cost of an event bracket with no kernel in it: the median of the brackets that are empty ("(empty)" and the
    unused split-K slots), i.e. of those within 1 us of the shortest one."""
    cands = sorted([ms for name, ms in stages if name == "(empty)" or name.endswith("#splitk_reduce")])
    near = [ms for ms in cands if ms <= cands[0] + 1e-3]
    return near[len(near) // 2]


def aggregate_stages(stages, ops, n, frame_bytes, size, hp_blocks, inner):
    """Event-bracketed stage times -> per-kernel-class totals.  A network stage's bracket holds `inner` back-to-back
    launches (wz_profile_stages): (bracket - empty bracket) / inner = one launch including its in-stream boundary."""
    from watsor_amd import arch
    by_name = {o["name"]: o for o in ops}
    mb_index = {o["name"]: i for i, o in enumerate([o for o in ops if o["kind"] == arch.OP_MBCONV])}
    overhead = empty_bracket_ms(stages)
    agg = {}

    def slot(k):
        return agg.setdefault(k, dict(ms=0.0, flops=0.0, bytes=0.0, launches=0, min_bytes=0.0))

    # split blocks that ran as TWO launches (csrc/k_mbconv_hp2.hip: blocks 13 .. 16 of the robust program from four frames up): the op's own slot holds
    # launch A (expand + depthwise), its "#splitk_reduce" slot launch B (the project GEMM); the per-layer rule's bytes are dealt accordingly
    two_launch = set()
    for name, ms in stages:
        base = name[:-len("#splitk_reduce")] if name.endswith("#splitk_reduce") else None
        if base in by_name and by_name[base]["kind"] == arch.OP_MBCONV and mb_index.get(base, 1 << 30) < hp_blocks and \
                by_name[base]["wout"] <= 10 and max(ms - overhead, 0.0) / inner >= 5e-4:
            two_launch.add(base)

    def project_cost(o):
        M = n * o["hout"] * o["wout"]
        return 2.0 * M * o["cmid"] * o["cout"], 2.0 * (M * o["cmid"] + o["cmid"] * o["cout"] + M * o["cout"])

    for name, ms in stages:
        post = name.startswith("post/") or name in ("(empty)", "h2d_descriptors")
        ms = max(ms - overhead, 0.0) / (1 if post else inner)
        if name.endswith("#splitk_reduce") and name[:-len("#splitk_reduce")] in two_launch:
            o = by_name[name[:-len("#splitk_reduce")]]
            fl, by = project_cost(o)
            a = slot("wz_k_hp2_proj")
            a["ms"] += ms; a["flops"] += fl; a["bytes"] += by; a["launches"] += 1
            a["min_bytes"] += 4.0 * (n * o["hout"] * o["wout"] * o["cmid"] + o["cmid"] * o["cout"]) + (2.0 if o["name"].endswith("_16") else 4.0) * n * o["hout"] * o["wout"] * o["cout"]
            continue
        if name in two_launch:
            o = by_name[name]
            fl, by = algorithmic_cost(o, n)
            pf, pb = project_cost(o)
            a = slot("wz_k_hp2_expdw")
            a["ms"] += ms; a["flops"] += fl - pf; a["bytes"] += by - pb; a["launches"] += 1
            a["min_bytes"] += 4.0 * (n * o["hin"] * o["win"] * o["cin"] + o["cin"] * o["cmid"] + 9 * o["cmid"] + n * o["hout"] * o["wout"] * o["cmid"])
            continue
        if name.endswith("#splitk_reduce"):
            k, fl, by = "wz_k_splitk_reduce", 0.0, 0.0
            if ms < 5e-4:
                continue
            mb = None
        elif name in ("heads#small_convs", "heads#big_convs"):   # the SSD heads' shared launches: their flops / bytes are
            k, fl, by, mb = "wz_k_conv<3>", 0.0, 0.0, None       # counted in their own (empty) op slots below
            if ms < 5e-4:
                continue
        elif name in by_name:
            o = by_name[name]
            mb = mb_index.get(name)
            k = kernel_class(o, mb is not None and mb < hp_blocks)
            fl, by = algorithmic_cost(o, n)
            if ms < 5e-4 and o["kind"] == arch.OP_CONV:     # deferred into the shared launch: work yes, launch no
                a = slot(k)
                a["flops"] += fl; a["bytes"] += by; a["min_bytes"] += by
                continue
        elif name == "preprocess":
            k, fl, mb = "wz_k_preprocess", 0.0, None
            by = float(n * (frame_bytes + size * size * 4 * 2 * (2 if hp_blocks else 1)))
        elif name.startswith("post/"):
            k, fl, by, mb = "wz_k_" + name.split("/")[1], 0.0, 0.0, None
            if ms < 5e-4:
                continue
        else:
            continue
        a = slot(k)
        a["ms"] += ms; a["flops"] += fl; a["bytes"] += by; a["launches"] += 1
        if mb is not None:
            a["min_bytes"] += fused_min_bytes(by_name[name], n, mb < hp_blocks, mb < hp_blocks - 1)
        else:
            a["min_bytes"] += by
    table = []
    for k, a in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
        t = a["ms"] * 1e-3
        t_hbm = a["bytes"] / (HBM_PEAK_GBS * 1e9)
        t_mfma = a["flops"] / (MFMA_PEAK_TFLOPS * 1e12)
        table.append(dict(kernel=k, launches=a["launches"], ms_per_step=a["ms"], avg_us=a["ms"] * 1e3 / a["launches"],
                          gbs=a["bytes"] / t / 1e9 if t > 0 else 0.0, tflops=a["flops"] / t / 1e12 if t > 0 else 0.0,
                          t_roof_frac=max(t_hbm, t_mfma) / t if t > 0 else 0.0,
                          bound="mfma" if t_mfma > t_hbm else "hbm",
                          bytes_per_launch=a["bytes"] / a["launches"], flops_per_launch=a["flops"] / a["launches"],
                          min_bytes_per_launch=a["min_bytes"] / a["launches"],
                          min_gbs=a["min_bytes"] / t / 1e9 if t > 0 else 0.0))
    return table, overhead


def roofline_object(table, overhead, single_table, inner, robust=False):
    """The JSON `roofline` object for the dominant kernel class of the step."""
    dom = table[0]
    if dom["bound"] == "hbm":
        ach, peak, unit = dom["gbs"], HBM_PEAK_GBS, "GB/s"
    else:
        ach, peak, unit = dom["tflops"], MFMA_PEAK_TFLOPS, "TFLOP/s"
    traffic = pmc_traffic(dom["kernel"])
    roof = dict(kernel=dom["kernel"], bound=dom["bound"], achieved=round(ach, 3), peak=peak, unit=unit,
                frac=round(ach / peak, 5), traffic=traffic,
                avg_launch_us=round(dom["avg_us"], 3), launches_per_step=dom["launches"],
                duration_method="HIP events on the lane's stream around %d back-to-back launches of each kernel "
                                "(wz_profile_stages), empty bracket %.2f us subtracted, / %d: a launch incl. its in-stream "
                                "boundary" % (inner, overhead * 1e3, inner),
                algorithmic_bytes_per_launch=round(dom["bytes_per_launch"]),
                algorithmic_flops_per_launch=round(dom["flops_per_launch"]),
                # what the launch has to move when intermediate tensors stay on chip (= algorithmic for unfused kernels)
                fused_min_bytes_per_launch=round(dom["min_bytes_per_launch"]),
                frac_fused_min=round(dom["min_gbs"] / HBM_PEAK_GBS, 5))
    if traffic:      # bytes the memory-side counters saw per launch (committed rocprofv3 --pmc passes) at this run's duration
        roof["frac_counter_traffic"] = round(traffic["bytes"] / (dom["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)
    single = {r["kernel"]: r for r in single_table}.get(dom["kernel"])
    if single:       # the same kernel with ONE launch per bracket (the cost of the event pair estimated, not amortised)
        roof["avg_launch_us_single_bracket"] = round(single["avg_us"], 3)
    sk = skeleton_ratio(dom["kernel"], dom["launches"], robust)
    if sk:           # what the same launches take with their arithmetic removed (committed measurement, profiles/hp_skeleton.json): the
        roof["arithmetic_free_skeleton"] = sk      # ceiling of THIS decomposition into tiles and chunks -- frac could rise by that ratio at most
        roof["frac_if_arithmetic_were_free"] = round(roof["frac"] * sk["real_over_skeleton"], 5)
    rp = rocprof_avg_us(dom["kernel"])
    if rp:           # ... and at the duration the committed rocprofv3 kernel trace of this command reports
        roof["avg_launch_us_rocprof"] = rp
        roof["frac_at_rocprof_duration"] = round(roof["frac"] * dom["avg_us"] / rp, 5)
    # What bounds the fraction on THIS workload, each term with the measurement behind it (round 5): at batch 8 a layer's
    # roofline time is shorter than the dependency wait between two kernels of one stream, and the launches of the 10x10 maps cannot be
    # shorter than the weight stream of one of their workgroups.
    step_bytes = sum(r["bytes_per_launch"] * r["launches"] for r in table if r.get("bytes_per_launch"))
    roof["limits"] = dict(
        whole_step_algorithmic_bytes=round(step_bytes),
        whole_step_us_at_hbm_peak=round(step_bytes / (HBM_PEAK_GBS * 1e9) * 1e6, 1),
        # the entries below are STATIC: read off committed profiles of round 6, not measured by this run
        static_from_profiles=True,
        in_stream_boundary_us=2.0, boundaries_per_step=30,
        boundary_source="profiles/r06zz_boundary_in_engine_graph.txt (in-kernel stamps, one lane): 60.9 us of gaps over the 30 boundaries of a lone batch; "
                        "profiles/r06_boundary_microbench.txt: 1.05 us between trivial kernels of a captured graph on the same box, + 0.125 us per MB the predecessor leaves dirty",
        frac_ceiling_of_one_lane_with_free_kernels=round(step_bytes / (HBM_PEAK_GBS * 1e9) * 1e6 / (step_bytes / (HBM_PEAK_GBS * 1e9) * 1e6 + 61.0), 3),
        cu_stream_gbs=130.0,
        cu_stream_source="profiles/r05_cu_stream_microbench.txt (tools/micro/cu_stream.hip): one CU pulls L2-resident bytes at 110 - 143 GB/s -- what sized the "
                         "two-launch form of blocks 13 .. 16 (<= 0.25 MB per workgroup instead of 1.2 - 1.8 MB)")
    return roof


def pmc_traffic(kernel):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes of this same command
    (profiles/pmc_traffic.json, written by tools/pmc_summary.py from separate --pmc FETCH_SIZE / WRITE_SIZE runs;
    FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for 16 B/lane reads on gfx950).  None when absent."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        t = json.load(open(path)).get(kernel)
        if not t or t["fetch_bytes_corrected"] is None or t["write_bytes"] is None:
            return None
        return dict(bytes=round(t["fetch_bytes_corrected"] + t["write_bytes"]), fetch_bytes_raw=round(t["fetch_bytes_raw"]),
                    fetch_bytes_corrected=round(t["fetch_bytes_corrected"]), write_bytes=round(t["write_bytes"]),
                    source="profiles/pmc_traffic.json (rocprofv3 --pmc of this command, mean per launch; committed, not of this run)")
    except (OSError, ValueError, KeyError):
        return None


def kernel_class_of(name):
    """rocprofv3's kernel name -> the class names used in this file."""
    k = name.replace("void ", "").split("(")[0]
    base = k.split("<")[0]
    if base.startswith("_Z"):
        return "wz_k_preprocess" if "preprocess" in base else "wz_k_stem" if "stem" in base else base
    if base.startswith("wz_k_mbconv_hp"):
        return "wz_k_mbconv_hp"
    if base.startswith("wz_k_mbconv"):
        return "wz_k_mbconv"
    if base in ("wz_k_conv_lds", "wz_k_conv"):
        return "wz_k_conv<%s>" % k.split("<")[1].split(",")[0].split(">")[0]
    return base


def live_pmc_traffic(timeout_s=60):
    """HBM-side bytes per launch and kernel class, measured NOW: two `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE --
    they do not fit one pass, MI355X_MICROARCH.md) over a short single-lane run of this same file (`--pmc-child`).
    FETCH_SIZE is doubled as the guide prescribes for 16 B/lane reads on gfx950 (it tallies a 128-B request as 64 B);
    both counters are reported in KiB.  Returns {class: {...}} or None when rocprofv3 is not usable here."""
    import glob
    import shutil
    import sqlite3
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.isfile("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None
    sums = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="wz_pmc_", dir="/tmp")
        try:
            env = dict(os.environ, TMPDIR="/tmp", WZ_LANES="1", WZ_BENCH_VERBOSE="0")
            p = subprocess.run([exe, "--pmc", counter, "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
                                "--pmc-child"], cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                               timeout=timeout_s)
            dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
            if p.returncode != 0 or not dbs:
                return None
            db = sqlite3.connect(dbs[0])
            for kname, value in db.execute("select kernel_name, value from counters_collection where counter_name = ?", (counter,)):
                a = sums.setdefault(kernel_class_of(kname), {}).setdefault(counter, [0.0, 0])
                a[0] += value
                a[1] += 1
            db.close()
        except (subprocess.TimeoutExpired, OSError, sqlite3.Error):
            return None
        finally:
            shutil.rmtree(d, ignore_errors=True)
    out = {}
    for k, c in sums.items():
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            f = c["FETCH_SIZE"][0] / c["FETCH_SIZE"][1] * 1024.0
            w = c["WRITE_SIZE"][0] / c["WRITE_SIZE"][1] * 1024.0
            out[k] = dict(bytes=round(2 * f + w), fetch_bytes_raw=round(f), fetch_bytes_corrected=round(2 * f), write_bytes=round(w),
                          launches_sampled=c["FETCH_SIZE"][1],
                          source="rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, two passes of this run (single lane), mean per launch")
    return out or None


def schedule_child():
    """The headline workload under whatever WZ_SCHEDULE the parent put into the environment (the library reads it once per process):
    one JSON line {value, p50_ms}."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    d = "/tmp/wz_sched_child_%d" % os.getpid()
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    weights = synthetic_weights(1234)
    builder.save_engine(builder.build_engine(weights, **HEADLINE_PROGRAM), path)
    eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), BATCH, WIDTH, HEIGHT)
    try:
        hfr = [synthetic_frame(WIDTH, HEIGHT, 1234 + i) for i in range(RING * BATCH)]
        dfr = [eng.upload(f) for f in hfr]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, dfr[(s % RING) * BATCH:(s % RING + 1) * BATCH], [WIDTH] * BATCH, [HEIGHT] * BATCH),
                       BATCH, steps=400, warm=40)
        r["graph_nodes_per_batch"] = eng.graph_nodes(0)
        r["schedule"] = eng.schedule
        # the rows THIS schedule's launch shapes produce, against the oracle (three of the batch's frames: ~2 s of oracle each)
        pr = parity_leg(eng, hfr, dfr, weights, check=(0, 3, 7))
        r["parity"] = {k: pr[k] for k in ("max_dscore", "max_dbox_px", "frames", "rows_compared", "rows_unexplained", "within_tolerance")}
        # ... and the load this schedule is FOR (what the factory's `schedule: auto` selects for up to 4 cameras per detector): one camera's
        # frame at a time -- configs[2]'s share of a GPU with its frames in HBM, and the plugin call on one pageable host frame
        eng.close()
        eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), 4, 1280, 720)
        f720 = [eng.upload(synthetic_frame(1280, 720, 600 + i)) for i in range(5)]
        one = throughput(eng, lambda lane, s: eng.submit_device(lane, [f720[s % 5]], [1280], [720]), 1, steps=300, warm=20)
        r["config3_1x720p_b1"] = dict(value=one["value"], unit="frames/s", p50_ms=one["p50_ms"])
        from watsor_amd.detection.hip_gpu import HipObjectDetector
        from watsor_amd.runtime import ROW_DTYPE
        eng.close()
        eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), 4, WIDTH, HEIGHT)
        r["host_frames_pinned_lone_batch_b4"] = lone_host_batch(eng, hfr)
        eng.close()
        with HipObjectDetector(d, int(os.environ.get("LOCAL_RANK", "0")), max_batch=1, max_width=WIDTH, max_height=HEIGHT) as det:
            rows = np.zeros(100, ROW_DTYPE)
            for _ in range(20):
                det.detect(hfr[0].shape, hfr[0], rows)
            ms = [det.detect(hfr[i % len(hfr)].shape, hfr[i % len(hfr)], rows) for i in range(300)]
            r["plugin_detect_b1"] = dict(p50_ms=round(float(np.median(ms)), 4), p99_ms=round(float(np.percentile(ms, 99)), 4))
        print(json.dumps(r), flush=True)
    finally:
        try:
            eng.close()
        except Exception:
            pass
        os.remove(path)
        os.rmdir(d)
    return 0


def latency_schedule_leg():
    """WZ_SCHEDULE=latency: the launch shapes that finish a lone batch soonest (include/watsor_hip.h), measured in a child process on
    the headline workload -- what the default (throughput) schedule trades away."""
    env = dict(os.environ, WZ_SCHEDULE="latency", WZ_BENCH_VERBOSE="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--schedule-child"], env=env, capture_output=True, text=True, timeout=240)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        return dict(error=(p.stderr or p.stdout)[-300:])
    r = json.loads(lines[-1])
    r["workload"] = ("the headline workload with the LATENCY schedule (child process; `hip_options={'schedule': 'latency'}`, what `auto` picks for up "
                     "to 4 cameras per detector) + the single-frame operating points it is for: configs[2]'s share with frames in HBM, detect() of one host frame")
    return r


def pmc_child():
    """The workload the two counter passes of `live_pmc_traffic` profile: 12 batches on one lane, nothing else."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    d = "/tmp/wz_pmc_child_%d" % os.getpid()
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    builder.save_engine(builder.build_engine(synthetic_weights(1234), **HEADLINE_PROGRAM), path)
    eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), BATCH, WIDTH, HEIGHT)
    try:
        fr = [eng.upload(synthetic_frame(WIDTH, HEIGHT, 1234 + i)) for i in range(BATCH)]
        for _ in range(12):
            eng.submit_device(0, fr, [WIDTH] * BATCH, [HEIGHT] * BATCH)
            eng.wait(0)
    finally:
        eng.close()
        os.remove(path)
        os.rmdir(d)


def skeleton_ratio(kernel, launches, robust=False):
    """The committed skeleton measurement of the dominant kernel (profiles/hp_skeleton.json, from profiles/r04_hp_skeleton.txt): real / skeleton duration."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "hp_skeleton.json"))).get(kernel)
        if robust and launches == t["robust_program_blocks_0_12"]["launches"]:
            prog = t["robust_program_blocks_0_12"]
        else:
            prog = t["robust_program"] if launches == t["robust_program"]["launches"] else t["default_program"]
        return dict(avg_us_real=prog["avg_us_real"], avg_us_skeleton=prog["avg_us_skeleton"],
                    real_over_skeleton=round(prog["avg_us_real"] / prog["avg_us_skeleton"], 3), source=t["source"])
    except (OSError, ValueError, KeyError, TypeError):
        return None


def lane_overlap(timeout_s=120):
    """Kernels in flight and CU-slot-time per step of the headline workload, from in-kernel entry / exit stamps of an UNPROFILED four-lane
    run (tools/lane_overlap.py on libwatsor_hip_stamps.so -- `make -C watsor_amd/csrc stamps`; rocprofv3's kernel trace serialises the
    lanes: concurrency 1.18 under it).  Live when the stamps library is there, else the committed profiles/lane_overlap.json."""
    keep = ("kernels_in_flight_mean_while_busy", "time_share_by_kernels_in_flight", "chip_idle_share", "cu_slot_time_us_per_step",
            "cu_slot_time_uncapped_us_per_step", "kernel_time_sum_us_per_step", "us_per_step_device_clock", "slot_time_over_step_time",
            "frames_per_s_stamped_run", "frames_per_s_product_library", "launches_per_step", "lanes", "program")
    res, source = None, None
    tool = os.path.join(ROOT, "tools", "lane_overlap.py")
    if os.path.isfile(os.path.join(ROOT, "watsor_amd", "libwatsor_hip_stamps.so")):
        tmp = "/tmp/wz_lane_overlap_%d.json" % os.getpid()
        try:
            p = subprocess.run([sys.executable, tool, "--steps", "400", "--json", tmp], capture_output=True, text=True, timeout=timeout_s)
            if p.returncode == 0 and os.path.isfile(tmp):
                res, source = json.load(open(tmp)), "live: tools/lane_overlap.py in this run (in-kernel stamps, no profiler)"
        except (subprocess.TimeoutExpired, OSError, ValueError):
            res = None
        finally:
            if os.path.isfile(tmp):
                os.remove(tmp)
    if res is None:
        try:
            res, source = json.load(open(os.path.join(ROOT, "profiles", "lane_overlap.json"))), "committed profiles/lane_overlap.json"
        except (OSError, ValueError):
            return None
    out = {k: res[k] for k in keep if k in res}
    out["largest_holders"] = [dict(launch=p_["launch"], kernel=p_["kernel"][:48], workgroups=p_["workgroups"], wg_per_cu=p_["wg_per_cu"],
                                   mean_us=p_["mean_us"], slot_time_us=p_["slot_time_us"])
                              for p_ in sorted(res.get("per_launch", []), key=lambda q: -q["slot_time_us"])[:6]]
    out["source"] = source
    return out


def rocprof_avg_us(kernel):
    """Average per-dispatch duration of `kernel` in the committed rocprofv3 kernel trace of this command
    (profiles/rocprof_kernel_avg.json)."""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "rocprof_kernel_avg.json"))).get(kernel, {}).get("avg_us")
    except (OSError, ValueError):
        return None


# --------------------------------------------------------------------------------------------------
# legs
# --------------------------------------------------------------------------------------------------
def throughput(eng, submit, n_frames_per_step, steps=400, warm=40):
    """frames/s of `steps` asynchronous steps over the engine's lanes + p50 of synchronous ones."""
    lanes = eng.num_slots
    for s in range(warm):
        submit(s % lanes, s)
    eng.sync()
    t0 = time.perf_counter()
    for s in range(steps):
        submit(s % lanes, s)
    eng.sync()
    dt = time.perf_counter() - t0
    lat = []
    for s in range(min(steps, 60)):
        t1 = time.perf_counter()
        submit(0, s)
        eng.wait(0)
        lat.append((time.perf_counter() - t1) * 1e3)
    return dict(value=round(steps * n_frames_per_step / dt, 1), unit="frames/s", ms_per_step=round(dt / steps * 1e3, 4),
                p50_ms=round(float(np.median(lat)), 4), frames_per_step=n_frames_per_step, steps=steps)


def lone_host_batch(eng, host_frames, n=4, reps=200):
    """A LONE batch of n page-locked 640x480 host frames, submit + collect, nothing else in flight -- what a detector with up to four
    cameras does all day (one queued frame per camera, `watsor/stream/sync.py:156-166`): p50 / p99 in ms."""
    from watsor_amd.runtime import ROW_DTYPE
    arena = np.ascontiguousarray(np.stack(host_frames[:2 * n]))
    eng.host_register(arena)
    try:
        rows = [np.zeros(100, ROW_DTYPE) for _ in range(n)]
        lat = []
        for i in range(reps + 20):
            views = [arena[(i % 2) * n + k] for k in range(n)]
            t1 = time.perf_counter()
            eng.submit_host(0, views)
            eng.collect(0, rows)
            if i >= 20:
                lat.append((time.perf_counter() - t1) * 1e3)
        return dict(p50_ms=round(float(np.median(lat)), 4), p99_ms=round(float(np.percentile(lat, 99)), 4), frames=n)
    finally:
        eng.sync()
        eng.host_unregister(arena)


def sample_detect_config(nz):
    """Thresholds of the reference's sample camera (`config/config.yaml:69-79`); zones limited to those the mask has."""
    return [{"person": {"area": 20, "confidence": 60, "zones": []}},
            {"car": {"area": 10, "confidence": 50, "zones": [z for z in (1, 3, 5) if z <= nz]}},
            {"truck": {"area": 10, "confidence": 50, "zones": []}}]


def config_legs(engine_path, device, rank, weights=None):
    """Per-GPU shares of BASELINE.json configs[2..4] (frames resident in HBM, filters on where the config has them)
    plus the north star's 300x300 sweep point."""
    from watsor_amd.filter.hip_filter import HipCameraFilter
    from watsor_amd.runtime import HipEngine, zones_from_alpha
    from watsor_amd.synth import synthetic_frame, synthetic_zone_mask
    legs = {}
    eng = HipEngine(engine_path, device, 16, 1920, 1080)
    try:
        # north star sweep point: synthetic 300x300 frames, batch 8
        f300 = [eng.upload(synthetic_frame(300, 300, 500 + i)) for i in range(8)]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, f300, [300] * 8, [300] * 8), 8)
        r["workload"] = "synthetic 300x300 frames in HBM, batch 8"
        legs["frame_300x300_b8"] = r
        # configs[2]: 8 x 1280x720 streams, one camera per GPU -> this GPU's share: ONE camera; its frames arrive one at a
        # time (BalancedQueue holds one queued frame per camera, watsor/stream/sync.py:156-166), so batch = 1 per lane
        f720 = [eng.upload(synthetic_frame(1280, 720, 600 + i)) for i in range(5)]      # 5 frames over 4 lanes: no lane replays a scene
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, [f720[s % 5]], [1280], [720]), 1, steps=300, warm=20)
        r["workload"] = "configs[2] share: 1 camera 1280x720, batch 1 on each of %d lanes, frames in HBM" % eng.num_slots
        legs["config3_1x720p_b1"] = r
        h720 = synthetic_frame(1280, 720, 600)
        if weights is not None:      # live parity of this leg's configuration (one 720p frame per batch): its rows against the oracle
            try:
                eng.submit_device(0, [f720[0]], [1280], [720])
                eng.wait(0)
                pr = rows_parity(eng.slot_rows(0, 1).copy(), [h720], weights, check=(0,))
                r["parity"] = {k: pr[k] for k in ("max_dscore", "max_dbox_px", "frames", "rows_compared", "rows_unexplained", "within_tolerance")}
            except Exception as e:
                r["parity"] = dict(error=repr(e))
        # configs[3]: 32 x 1920x1080 cameras with per-camera alpha zone masks, 4 cameras per GPU: one frame of each per step
        filters = []
        masks = [synthetic_zone_mask(1920, 1080, 100 + c, 2 + c % 5) for c in range(8)]
        for c in range(4):
            nz = zones_from_alpha(masks[c])[0].shape[0]
            filters.append(HipCameraFilter(eng, c, {"width": 1920, "height": 1080, "detect": sample_detect_config(nz)}, alpha=masks[c]))
        h1080 = [synthetic_frame(1920, 1080, 700 + c) for c in range(8)]
        f1080 = [eng.upload(f) for f in h1080]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, f1080[:4], [1920] * 4, [1080] * 4, cams=[0, 1, 2, 3]), 4)
        r["workload"] = "configs[3] share: 4 cameras 1920x1080, each with its alpha zone mask + sample-config thresholds (filters on), batch 4, frames in HBM"
        legs["config4_4x1080p_masks_b4"] = r
        if weights is not None:      # live parity: one of the four 1080p frames' rows against the oracle, all four cameras' zones[] bit for bit
            try:
                eng.submit_device(0, f1080[:4], [1920] * 4, [1080] * 4, cams=[0, 1, 2, 3])
                eng.wait(0)
                got4 = eng.slot_rows(0, 4).copy()
                pr = rows_parity(got4, h1080[:4], weights, check=(2,))
                r["parity"] = {k: pr[k] for k in ("max_dscore", "max_dbox_px", "frames", "rows_compared", "rows_unexplained", "within_tolerance")}
                r["parity"]["zones_bit_exact"] = zones_bit_exact(got4, [0, 1, 2, 3], {c: (1920, 1080, masks[c]) for c in range(4)})
            except Exception as e:
                r["parity"] = dict(error=repr(e))
        # configs[4]: 128 mixed cameras (640x480 / 1920x1080) with masks + confidence / area filters: 16 per GPU, saturation
        small_masks = [synthetic_zone_mask(640, 480, 300 + c, 2 + c % 5) for c in range(8)]
        hsmall = [synthetic_frame(640, 480, 800 + c) for c in range(8)]
        fsmall = [eng.upload(f) for f in hsmall]
        for c in range(4, 8):
            nz = zones_from_alpha(masks[c])[0].shape[0]
            filters.append(HipCameraFilter(eng, c, {"width": 1920, "height": 1080, "detect": sample_detect_config(nz)}, alpha=masks[c]))
        for c in range(8):
            nz = zones_from_alpha(small_masks[c])[0].shape[0]
            filters.append(HipCameraFilter(eng, 8 + c, {"width": 640, "height": 480, "detect": sample_detect_config(nz)}, alpha=small_masks[c]))
        mix_frames, mix_w, mix_h, mix_c, mix_host = [], [], [], [], []
        for c in range(8):                         # alternating resolutions, as the config says
            mix_host += [hsmall[c], h1080[c]]
            mix_frames += [fsmall[c], f1080[c]]
            mix_w += [640, 1920]
            mix_h += [480, 1080]
            mix_c += [8 + c, c]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, mix_frames, mix_w, mix_h, cams=mix_c), 16, steps=80, warm=8)
        r["workload"] = ("configs[4] share: 16 cameras alternating 640x480 / 1920x1080, masks + confidence / area thresholds "
                         "(config.yaml:69-79), batch 16 = one frame of each camera, frames in HBM, saturation")
        legs["config5_16_mixed_filters_b16"] = r
        if weights is not None:
            # parity of THIS leg's configuration: batch 16 (the grid shapes `hip_detector_options` selects for more than 8 cameras), mixed
            # resolutions, camera filters on -- four of the sixteen frames' rows (label, score, box) against the oracle, and every
            # frame's zones[] / pass bytes against the oracle's literal polygon filters on those rows (bit-exact or not at all)
            try:
                eng.submit_device(0, mix_frames, mix_w, mix_h, cams=mix_c)
                eng.wait(0)
                got = eng.slot_rows(0, 16).copy()
                pr = rows_parity(got, mix_host, weights, check=(0, 1, 10, 15))
                r["parity"] = {k: pr[k] for k in ("max_dscore", "max_dbox_px", "frames", "rows_compared", "rows_unexplained", "within_tolerance")}
                r["parity"]["zones_bit_exact"] = zones_bit_exact(got, mix_c, {8 + c: (640, 480, small_masks[c]) for c in range(8)} |
                                                                 {c: (1920, 1080, masks[c]) for c in range(8)})
            except Exception as e:                     # a leg must not take the headline down with it
                r["parity"] = dict(error=repr(e))
        for f in filters:
            f.close()
    finally:
        eng.close()
    return legs


def zones_bit_exact(rows, cams, cam_masks):
    """The rows' zones[] as the GPU wrote them == the oracle's literal MaskFilter (polygon test, oracle/filters.py) on the same rows,
    for every frame of the batch (north star: "zone-mask hit/miss is bit-exact")."""
    from oracle import filters as of
    from oracle import zones as oz
    from watsor_amd.share import BoundingBox, Detection
    for i, cam in enumerate(cams):
        w, h, alpha = cam_masks[cam]
        nz = len(oz.zone_polygons(alpha))
        cfg = {"width": w, "height": h, "detect": sample_detect_config(nz)}
        chain = [of.ConfidenceFilter(cfg), of.AreaFilter(cfg), of.MaskFilter(cfg, alpha=alpha)]
        for r in rows[i]:
            d = Detection(label=int(r["label"]), confidence=float(r["confidence"]),
                          bounding_box=BoundingBox(int(r["x_min"]), int(r["y_min"]), int(r["x_max"]), int(r["y_max"])))
            _ = d.label > 0 and all(f(d) for f in chain)       # `label > 0 and Confidence and Area and Mask`, short-circuit (track.py:26)
            if list(d.zones) != [int(z) for z in r["zones"]]:
                return False
    return True


def host_legs(engine_path, model_dir, device, host_frames):
    """The reference's actual boundary: frames handed over as HOST memory (`detector.py:104-107`)."""
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.runtime import HipEngine, ROW_DTYPE
    legs = {}
    eng = HipEngine(engine_path, device, BATCH, WIDTH, HEIGHT)
    try:
        arena = np.ascontiguousarray(np.stack(host_frames[:2 * BATCH]))     # one "FrameBuffer arena", page-locked once
        eng.host_register(arena)
        try:
            views = [[arena[b * BATCH + i] for i in range(BATCH)] for b in range(2)]
            r = throughput(eng, lambda lane, s: eng.submit_host(lane, views[s % 2]), BATCH)
            r["workload"] = "640x480 frames in page-locked host memory (wz_host_register + wz_submit_host), batch 8: H2D inside the step"
            legs["host_frames_pinned_b8"] = r
        finally:
            eng.sync()
            eng.host_unregister(arena)
    finally:
        eng.close()
    # configs[3] / [4] put 1920x1080 cameras on a GPU: there the boundary is PCIe-bound (6.2 MB per RGB24 frame), and the
    # decoder side of SURVEY 8(f)-3 -- NV12 frames, converted inside the resize kernel -- halves the bytes
    from watsor_amd.runtime import FMT_NV12
    from watsor_amd.synth import synthetic_frame
    eng = HipEngine(engine_path, device, BATCH, 1920, 1080)
    try:
        big = [synthetic_frame(1920, 1080, 900 + i) for i in range(4)]
        for name, fmt, shape in (("rgb24", None, (1080, 1920, 3)), ("nv12", FMT_NV12, (1620, 1920))):
            arena = np.zeros((2 * BATCH,) + shape, np.uint8)
            for i in range(2 * BATCH):   # (pixel values do not matter to the transfer; the NV12 planes are the RGB bytes re-cut)
                arena[i] = big[i % 4].reshape(-1)[:arena[i].size].reshape(shape)
            eng.host_register(arena)
            try:
                views = [[arena[b * BATCH + i] for i in range(BATCH)] for b in range(2)]
                fmts = [fmt] * BATCH if fmt is not None else None
                r = throughput(eng, lambda lane, s: eng.submit_host(lane, views[s % 2], formats=fmts), BATCH, steps=60)
                r["bytes_per_frame"] = int(arena[0].size)
                r["workload"] = ("1920x1080 %s frames in page-locked host memory, batch 8, H2D inside the step" % name.upper()
                                 + ("" if fmt is None else " (colour conversion in the resize kernel; the decoder writes -pix_fmt nv12)"))
                legs["host_frames_pinned_1080p_%s_b8" % name] = r
            finally:
                eng.sync()
                eng.host_unregister(arena)
    finally:
        eng.close()
    eng = HipEngine(engine_path, device, 4, WIDTH, HEIGHT)
    try:
        legs["host_frames_pinned_lone_batch_b4"] = dict(lone_host_batch(eng, host_frames), schedule=eng.schedule,
                                                        workload="a lone batch of four 640x480 frames in page-locked host memory, submit + collect, nothing else in "
                                                                 "flight (a detector with four cameras); the latency schedule's twin: legs.latency_schedule_b8.host_frames_pinned_lone_batch_b4")
    finally:
        eng.close()
    # the plugin call the reference worker makes: one frame from (pageable) host memory, synchronous -- the time
    # `ObjectDetector._next_frame` feeds into `inference_time` (detector.py:107-109)
    with HipObjectDetector(model_dir, device, max_batch=1, max_width=WIDTH, max_height=HEIGHT) as det:
        rows = np.zeros(100, ROW_DTYPE)
        f = host_frames[0]
        for _ in range(20):
            det.detect(f.shape, f, rows)
        ms, wall = [], []
        for i in range(300):
            f = host_frames[i % len(host_frames)]
            t1 = time.perf_counter()
            ms.append(det.detect(f.shape, f, rows))
            wall.append((time.perf_counter() - t1) * 1e3)
        legs["plugin_detect_b1"] = dict(p50_ms=round(float(np.median(ms)), 4), p99_ms=round(float(np.percentile(ms, 99)), 4),
                                        p50_ms_python_wall=round(float(np.median(wall)), 4),
                                        value=round(1000.0 / float(np.mean(wall)), 1), unit="frames/s",
                                        workload="HipObjectDetector.detect() of one 640x480 frame in pageable host memory, synchronous "
                                                 "(what the reference's inference_time measures, detector.py:107-109)")
    return legs


def host_config_legs(engine_path, device):
    """BASELINE configs[2..4] as a Watsor install meets them (`watsor/stream/share.py:68-73` hands over HOST views): the
    cameras' frame buffers in page-locked host memory, described once (`wz_bind_frames`), a step = one frame of every
    camera, filters on where the config has them.  Per-GPU shares, like `config_legs` (which stages the frames in HBM)."""
    from watsor_amd.filter.hip_filter import HipCameraFilter
    from watsor_amd.runtime import HipEngine, ROW_DTYPE, zones_from_alpha
    from watsor_amd.synth import synthetic_frame, synthetic_zone_mask
    legs = {}
    eng = HipEngine(engine_path, device, 16, 1920, 1080)
    filters = []
    try:
        def camera_set(specs, frames_per_cam=3):
            """specs: [(w, h, cam id or -1, seed)] -> (arena list, table)"""
            arenas, pix, ws, hs, cams, rows = [], [], [], [], [], []
            for w, h, cam, seed in specs:
                a = np.stack([synthetic_frame(w, h, seed + k) for k in range(frames_per_cam)])
                r = np.zeros((frames_per_cam, 100), ROW_DTYPE)
                eng.host_register(a)
                arenas.append((a, r))
                for k in range(frames_per_cam):
                    pix.append(a[k].ctypes.data); ws.append(w); hs.append(h); cams.append(cam); rows.append(r[k].ctypes.data)
            eng.bind_frames(pix, ws, hs, [0] * len(pix), cams, rows)
            return arenas

        def release(arenas):
            eng.sync()
            eng.bind_frames([], [], [], [], [], [])
            for a, _ in arenas:
                eng.host_unregister(a)

        def bound_throughput(n_cams, frames_per_cam, **kw):
            def submit(lane, s):
                k = s % frames_per_cam
                eng.submit_bound(lane, [c * frames_per_cam + k for c in range(n_cams)])
            return throughput(eng, submit, n_cams, **kw)

        # configs[2] share: one 1280x720 camera
        ar = camera_set([(1280, 720, -1, 600)], 5)
        r = bound_throughput(1, 5, steps=300, warm=20)
        r["workload"] = "configs[2] share: 1 camera 1280x720 in page-locked host memory, batch 1 on each of %d lanes" % eng.num_slots
        legs["config3_1x720p_b1_host"] = r
        release(ar)
        # configs[3] share: 4 x 1920x1080 with zone masks + thresholds
        masks = [synthetic_zone_mask(1920, 1080, 100 + c, 2 + c % 5) for c in range(8)]
        for c in range(8):
            nz = zones_from_alpha(masks[c])[0].shape[0]
            filters.append(HipCameraFilter(eng, c, {"width": 1920, "height": 1080, "detect": sample_detect_config(nz)}, alpha=masks[c]))
        ar = camera_set([(1920, 1080, c, 700 + 10 * c) for c in range(4)])
        r = bound_throughput(4, 3, steps=60, warm=8)
        r["workload"] = "configs[3] share: 4 cameras 1920x1080 RGB24 in page-locked host memory (PCIe inside the step), zone masks + thresholds on, batch 4"
        legs["config4_4x1080p_masks_b4_host"] = r
        release(ar)
        # configs[4] share: 16 mixed cameras, masks + confidence / area
        small_masks = [synthetic_zone_mask(640, 480, 300 + c, 2 + c % 5) for c in range(8)]
        for c in range(8):
            nz = zones_from_alpha(small_masks[c])[0].shape[0]
            filters.append(HipCameraFilter(eng, 8 + c, {"width": 640, "height": 480, "detect": sample_detect_config(nz)}, alpha=small_masks[c]))
        specs = []
        for c in range(8):
            specs += [(640, 480, 8 + c, 800 + 10 * c), (1920, 1080, c, 700 + 10 * c)]
        ar = camera_set(specs)
        r = bound_throughput(16, 3, steps=40, warm=6)
        r["workload"] = ("configs[4] share: 16 cameras alternating 640x480 / 1920x1080 in page-locked host memory, masks + confidence / area "
                         "thresholds, batch 16 = one frame of each camera, saturation")
        legs["config5_16_mixed_filters_b16_host"] = r
        release(ar)
    finally:
        for f in filters:
            f.close()
        eng.close()
    return legs


def worker_legs(model_dir, device=0, only_8cams=False):
    """Frames/s through the detector WORKER LOOP (tools/worker_bench.py): a spawned process running `BatchedWorkerMixin` over
    shared-memory frame buffers fed through a real multiprocessing.Queue -- `watsor/detection/detector.py:84-112`,
    `watsor/stream/work.py:25-33`, `watsor/stream/sync.py:144-166`."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import worker_bench
    legs = {}

    def leg(name, **kw):
        try:
            legs[name] = worker_bench.run(model_dir, device=device, **kw)
        except Exception as e:                     # a leg must not take the headline down with it
            legs[name] = dict(error=repr(e))

    leg("worker_spawned_8cams", n_cams=8, seconds=3.0)
    if only_8cams:
        return legs
    leg("worker_spawned_16cams", n_cams=16, seconds=3.0)
    # configs[3..4] put 16+ cameras on a GPU: the worker drains up to max_batch payloads per turn without waiting, and the factory
    # sets max_batch 16 for more than 8 cameras (`hip_detector_options`) -- the leg above, with the limit held at 8, is the comparison
    leg("worker_spawned_16cams_max_batch16", n_cams=16, seconds=3.0, max_batch=16)
    leg("worker_spawned_32cams_max_batch16", n_cams=32, seconds=3.0, max_batch=16, producers=4)
    leg("worker_spawned_8cams_per_batch_descriptions", n_cams=8, seconds=2.0, frame_table=False)
    # the reference's multi-device topology on one GPU: two worker processes on ONE queue (watsor/main.py:414-418)
    leg("two_workers_one_queue_16cams", n_cams=16, seconds=3.0, workers=2, gpus=1)
    return legs


def all_rank_legs(engine_path, model_dir, local_rank, host_frames, dist, world, plan=None, rank_info=None):
    """world > 1: the HOST-side legs on EVERY rank at the same time (a barrier in front of each).  Replicas whose frames sit in HBM
    scale trivially; what an 8-GPU Watsor box shares is the host -- PCIe root complex, memory bandwidth, cores for the worker
    processes and their producers -- and that only shows when all ranks move host frames together.  -> {leg: [per-rank dict]}"""
    mine = {}
    plan = plan or [("host", lambda: host_legs(engine_path, model_dir, local_rank, host_frames)),
                    ("host_configs", lambda: host_config_legs(engine_path, local_rank)),
                    ("worker", lambda: worker_legs(model_dir, device=local_rank, only_8cams=True))]
    for name, fn in plan:
        dist.barrier()
        try:
            mine.update(fn())
        except Exception as e:
            mine[name] = dict(error=repr(e))
    if rank_info is not None:
        mine["_rank"] = rank_info                    # where this rank ran: GPU's PCI address, NUMA node, CPUs it was pinned to
    gathered = [None] * world
    dist.all_gather_object(gathered, mine)
    return gathered


def summarise_rank_legs(gathered):
    """[per-rank {leg: dict}] -> {leg: {per_rank: [frames/s], sum, min, p50_ms_per_rank, workload}}"""
    out = {}
    if any("_rank" in g for g in gathered):
        out["ranks"] = [g.get("_rank") for g in gathered]
    for name in gathered[0]:
        if name == "_rank":
            continue
        vals = [g.get(name, {}).get("value") for g in gathered]
        entry = dict(per_rank=vals)
        if all(isinstance(v, (int, float)) for v in vals):
            entry.update(sum=round(float(sum(vals)), 1), min=min(vals), unit="frames/s")
        p50 = [g.get(name, {}).get("p50_ms", g.get(name, {}).get("p50_ms_enqueue_to_latch")) for g in gathered]
        if any(v is not None for v in p50):
            entry["p50_ms_per_rank"] = p50
        errs = [g.get(name, {}).get("error") for g in gathered if g.get(name, {}).get("error")]
        if errs:
            entry["errors"] = errs
        entry["workload"] = gathered[0].get(name, {}).get("workload", gathered[0].get(name, {}).get("frame"))
        out[name] = entry
    return out


def busy_scene_leg(frames, rank):
    """The benchmark's random-init network puts ~170 scores above 0.3 in 4 classes: a light load for `wz_k_nms`.  The same
    weights with the class logits widened (`synthetic_weights(class_gain=1.3)`): ~800 above 0.3 in ~25 classes, several hundred
    first-band candidates in same-class clusters -- through the full graph, batch 8, frames in HBM."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import synthetic_weights
    d = "/tmp/wz_bench_busy_%d_%d" % (os.getpid(), rank)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    builder.save_engine(builder.build_engine(synthetic_weights(1234, class_gain=1.3), **HEADLINE_PROGRAM), path)
    eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), BATCH, WIDTH, HEIGHT)
    try:
        dfr = [eng.upload(f) for f in frames[:RING * BATCH]]
        nb = len(dfr) // BATCH
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, dfr[(s % nb) * BATCH:(s % nb + 1) * BATCH], [WIDTH] * BATCH, [HEIGHT] * BATCH), BATCH)
        rows = eng.slot_rows(0, BATCH)
        r["detections_per_frame_above_0.3"] = float((rows["confidence"] > 0.3).sum()) / BATCH
        r["workload"] = "640x480 frames in HBM, batch 8, class logits widened (class_gain 1.3): a busy scene for the NMS kernel"
        return r
    finally:
        eng.close()
        os.remove(path)
        os.rmdir(d)


def rows_parity(got, frames, weights, check=None, tol=SCORE_TOLERANCE):
    """Detection rows `got[i]` of `frames[i]` (host arrays) against the oracle's, for the frames in `check` (default: all): the north
    star's criterion as oracle/compare.py states it -- scores, boxes, and an explanation for every row without a partner."""
    from oracle.compare import box_tolerance_px, compare_rows
    from oracle.detect import OracleObjectDetector, rows_as_array
    det = OracleObjectDetector(weights=weights)
    check = list(range(len(frames))) if check is None else list(check)
    worst, worst_px, matched, total, odd, unexplained, reasons, px_ok = 0.0, 0, 0, 0, 0, 0, {}, True
    for i in check:
        b, c, s, _, _ = det.raw(frames[i])
        ref = rows_as_array(frames[i].shape, b, c, s)
        r = compare_rows(got[i], ref, frames[i].shape, tol=tol)
        matched += len(r["pairs"])
        total += r["rows_reference"]
        worst = max(worst, r["max_dscore"])
        worst_px = max(worst_px, r["max_dbox_px"])
        px_ok = px_ok and r["max_dbox_px"] <= box_tolerance_px(frames[i].shape[1], frames[i].shape[0])
        unexplained += r["unexplained"]
        for _, why in r["missing"] + r["extra"]:
            odd += 1
            key = (why or "UNEXPLAINED").split(":")[0].split("(")[0].strip()
            reasons[key] = reasons.get(key, 0) + 1
    return dict(max_dscore=round(worst, 6), max_dbox_px=int(worst_px), frames=len(check), rows_compared=matched, rows_reference=total,
                tolerance=tol, rows_without_partner=odd, rows_without_partner_reasons=reasons, rows_unexplained=unexplained,
                within_tolerance=bool(worst <= tol and px_ok and unexplained == 0 and matched >= 0.9 * total))


def parity_leg(eng, host_frames, d_frames, weights, check=None):
    """North star criterion (1), live, on the engine that was just timed: scores of its detection rows vs the oracle's
    on 8 of the benchmark's own frames."""
    from oracle.compare import box_tolerance_px
    n = BATCH
    eng.submit_device(0, d_frames[:n], [WIDTH] * n, [HEIGHT] * n)
    eng.wait(0)
    got = eng.slot_rows(0, n).copy()
    out = rows_parity(got, host_frames[:n], weights, check)
    out["box_tolerance_px"] = box_tolerance_px(WIDTH, HEIGHT)
    out["against"] = ("oracle (CPU restatement of the reference's TF detector, fp32), same frames, rows matched by label and IoU >= 0.9; "
                      "a row without a partner must sit at the top-100 cut or at an NMS tie within 2 x tolerance (oracle/compare.py)")
    return out


def fp32_engine_leg(weights, frames, rank):
    """Throughput of the `-p 32` engine (fp32 storage, exact-fp32 MFMA) on the same workload, for reference."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    d = "/tmp/wz_bench32_%d_%d" % (os.getpid(), rank)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    builder.save_engine(builder.build_engine(weights, precision=32), path)
    eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), BATCH, WIDTH, HEIGHT)
    try:
        dfr = [eng.upload(f) for f in frames[:BATCH]]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, dfr, [WIDTH] * BATCH, [HEIGHT] * BATCH), BATCH, steps=60, warm=8)
    finally:
        eng.close()
        os.remove(path)
        os.rmdir(d)
    r.update(dtype="f32", workload="the headline workload on the -p 32 engine (scores within 1e-5 of the CPU detector)")
    return r


def plain_fp16_leg(weights, frames, rank):
    """The same workload on the `--plain-fp16` program (no split operands): faster, but 3x outside the score tolerance."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    d = "/tmp/wz_bench16p_%d_%d" % (os.getpid(), rank)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    builder.save_engine(builder.build_engine(weights, hp_upto=-1), path)
    eng = HipEngine(path, int(os.environ.get("LOCAL_RANK", "0")), BATCH, WIDTH, HEIGHT)
    try:
        dfr = [eng.upload(f) for f in frames[:BATCH]]
        r = throughput(eng, lambda lane, s: eng.submit_device(lane, dfr, [WIDTH] * BATCH, [HEIGHT] * BATCH), BATCH)
        par = parity_leg(eng, frames, dfr, weights)
    finally:
        eng.close()
        os.remove(path)
        os.rmdir(d)
    r.update(dtype="f16", max_dscore=par["max_dscore"], within_tolerance=par["within_tolerance"],
             workload="the headline workload on the --plain-fp16 program: NOT parity-qualified, shown for the cost of the tolerance")
    return r


def default_program_leg(weights, frames, rank):
    """The DEFAULT `-p 16` program (blocks 0 .. 12 split, linear chunk buffer, blocks 13 .. 16 plain fp16) on the headline workload --
    what the builder packs for weights whose channels live at one scale, like this benchmark's -- and why it is not the headline: the
    scores of both programs against the oracle on weights whose channels are spread over 1.5 and 2.0 decades (watsor_amd/synth.py:
    spread_channel_scales -- what folding a trained BatchNorm does to the channel amplitudes)."""
    from watsor_amd import engine as builder
    from watsor_amd.runtime import HipEngine
    from watsor_amd.synth import spread_channel_scales
    d = "/tmp/wz_bench16d_%d_%d" % (os.getpid(), rank)
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, "mi355x.bin")
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    r = {}
    try:
        runs = [("headline", weights, {})]
        for dec in (1.5, 2.0):
            sw = spread_channel_scales(weights, dec)
            runs += [("default_%s" % str(dec).replace(".", "p"), sw, {}), ("robust_%s" % str(dec).replace(".", "p"), sw, dict(robust=True))]
        for name, w, kw in runs:
            builder.save_engine(builder.build_engine(w, **kw), path)
            eng = HipEngine(path, dev, BATCH, WIDTH, HEIGHT)
            try:
                dfr = [eng.upload(f) for f in frames[:RING * BATCH]]
                if name == "headline":
                    nb = len(dfr) // BATCH
                    r = throughput(eng, lambda lane, s: eng.submit_device(lane, dfr[(s % nb) * BATCH:(s % nb + 1) * BATCH], [WIDTH] * BATCH, [HEIGHT] * BATCH),
                                   BATCH, steps=600, warm=60)
                par = parity_leg(eng, frames, dfr, w)
            finally:
                eng.close()
            if name == "headline":
                r.update(dtype="f16", max_dscore=par["max_dscore"], max_dbox_px=par["max_dbox_px"], within_tolerance=par["within_tolerance"])
            else:
                prog, dec = name.split("_")
                r["max_dscore_%s_program_weights_spread_%s_decades" % (prog, dec)] = par["max_dscore"]
        r["channel_spread_decades_of_the_benchmark_weights"] = round(builder.channel_spread_decades(weights), 2)
    finally:
        if os.path.exists(path):
            os.remove(path)
        os.rmdir(d)
    r["workload"] = ("the headline workload on the DEFAULT -p 16 program (what `python -m watsor_amd.engine` builds when the folded weights keep their "
                     "channels within %.2f decades); max_dscore_*: both programs against the oracle on weights spread over 1.5 / 2.0 decades"
                     % builder.SPREAD_VALIDATED_DECADES)
    return r


def cpu_baseline(weights, frames, budget_s=12.0):
    """Oracle detector (kind 'port') on this host's cores over a bounded sample of the same frames, with the split
    between the network (torch-CPU convolutions) and the post-processing (numpy + pure-Python class-by-class NMS)."""
    import torch
    from oracle import postprocess as post
    from oracle import preprocess as pre
    from oracle.detect import OracleObjectDetector
    from watsor_amd.share import DetectionArray
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = min(cores, int(os.environ.get("WZ_CPU_BASELINE_THREADS", "64")))
    # post-processing in one global score order (held equal to the literal class-by-class version by
    # tests/test_oracle_postprocess_fast.py): the baseline should be bounded by the network like a real TF run, not by 90
    # Python loops; the literal version's time is printed in `split_ms` beside it
    det = OracleObjectDetector(weights=weights, fast_post=True)
    rows = DetectionArray()
    # the thread count that serves THIS workload best on this host (a 300x300 MobileNet does not scale to 64 threads:
    # more of them make it slower); `cores` reports the count used
    best = None
    for nthreads in sorted({c for c in (4, 8, 16, 32, cores) if c <= cores}):
        torch.set_num_threads(nthreads)
        det.detect(frames[0].shape, frames[0], rows)       # warm-up (thread pools, allocations)
        t1 = time.perf_counter()
        for f in frames[:3]:
            det.detect(f.shape, f, rows)
        dt3 = time.perf_counter() - t1
        if best is None or dt3 < best[0]:
            best = (dt3, nthreads)
    cores = best[1]
    torch.set_num_threads(cores)
    t0 = time.perf_counter()
    done = 0
    lat = []
    while True:
        f = frames[done % len(frames)]
        t1 = time.perf_counter()
        det.detect(f.shape, f, rows)
        lat.append((time.perf_counter() - t1) * 1e3)
        done += 1
        if time.perf_counter() - t0 >= budget_s and done >= 4:
            break
    dt = time.perf_counter() - t0
    # where the time goes (4 frames, outside the sample above)
    t_pre = t_net = t_post = t_lit = 0.0
    anchors = post.anchors_center_size(post.generate_anchors(300))
    for f in frames[:4]:
        t1 = time.perf_counter()
        x = pre.preprocess(f, 300)[None]
        t2 = time.perf_counter()
        be, cl, _ = det._net.forward(x)
        t3 = time.perf_counter()
        post.postprocess(be[0], cl[0], anchors, fast=True)
        t4 = time.perf_counter()
        post.postprocess(be[0], cl[0], anchors)
        t5 = time.perf_counter()
        t_pre += t2 - t1; t_net += t3 - t2; t_post += t4 - t3; t_lit += t5 - t4
    return dict(value=round(done / dt, 3), unit="frames/s", cores=cores, kind="port",
                p50_ms=round(float(np.median(lat)), 2),
                split_ms=dict(resize_normalise=round(t_pre / 4 * 1e3, 2), network=round(t_net / 4 * 1e3, 2),
                              postprocess=round(t_post / 4 * 1e3, 2), postprocess_literal_checker=round(t_lit / 4 * 1e3, 2)),
                network_only_frames_per_s=round(4.0 / t_net, 2),
                sample="%d synthetic %dx%d frames, oracle (torch-CPU fp32 restatement of the reference TF detector, post-processing "
                       "in one global score order -- equal to the literal class-by-class checker, which takes "
                       "postprocess_literal_checker ms), %.1f s" % (done, WIDTH, HEIGHT, dt),
                published_reference="README.md:455 quotes ~24 FPS for the TF CPU detector (v1 model) on a desktop CPU")


def dump_outputs(rows, out_dir):
    """What the timed path handed back in one step: the rows of its batch (ROW_DTYPE [batch, 100]), every field but the padding as
    `out_dir/<field>.npy`, float64 (labels, zone flags and pixel coordinates are small integers: exact)."""
    os.makedirs(out_dir, exist_ok=True)
    for name in rows.dtype.names:
        if not name.startswith("_"):
            np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(rows[name], dtype=np.float64))


class _StubEngine:
    """GPU-less stand-in used only by --dry-run: same surface as HipEngine, a step is a 2 ms sleep."""
    num_slots = 2
    input_size = 300
    device_name = "stub"

    def __init__(self, *a, **k):
        self._busy = {}

    def upload(self, arr):
        return 1

    def submit_device(self, slot, d, ws, hs, cams=None):
        self.wait(slot)
        self._busy[slot] = time.perf_counter() + 0.002

    def wait(self, slot):
        t = self._busy.get(slot, 0) - time.perf_counter()
        if t > 0:
            time.sleep(t)

    def sync(self):
        for s in list(self._busy):
            self.wait(s)

    def slot_rows(self, slot, n):
        return np.zeros((n, 100), dtype=[("confidence", "<f8")])

    def close(self):
        pass


T_START = time.perf_counter()


def note(msg):
    if os.environ.get("WZ_BENCH_VERBOSE", "1") != "0":
        print("[bench %7.2fs] %s" % (time.perf_counter() - T_START, msg), file=sys.stderr, flush=True)


RANK_START_TIMEOUT_S = 300     # rendezvous: a rank that is not there by then never will be (gloo's own default is 30 minutes; the first `import torch` on a fresh box can take two)
RANK_POLL_S = 0.2


def spawn_ranks(n, argv, poll_s=RANK_POLL_S):
    """`--gpus N` without a launcher: one process per device ordinal 0 .. N-1 (the reference starts one detector
    process per device, `watsor/detection/detector.py:34-50`); gloo rendezvous on 127.0.0.1 for the barrier and the
    max-over-ranks; rank 0's JSON line is this process's output.
    A WATCHDOG polls the children: the moment any rank exits non-zero (no such device, engine creation failed, out of memory ...)
    the others are killed and the run fails with that rank's code -- without it rank 0 would sit in the rendezvous or in a barrier
    until gloo's timeout, i.e. for the driver's whole budget."""
    import signal
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    out_file = tempfile.TemporaryFile()
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=out_file if r == 0 else subprocess.DEVNULL, start_new_session=True))
    failed = None
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
            if bad:
                failed = bad[0]
                break
            if all(c == 0 for c in codes):
                break
            time.sleep(poll_s)
    finally:
        for p in procs:                                   # (also on KeyboardInterrupt / a driver's SIGTERM: no orphan holds a GPU)
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)      # each rank leads its own session: its worker / producer children go with it
                except (ProcessLookupError, PermissionError):
                    p.kill()
        for p in procs:
            p.wait()
    if failed is not None:
        print("[bench] rank %d exited with code %d: the other ranks were stopped" % failed, file=sys.stderr, flush=True)
        return failed[1] if failed[1] > 0 else 1
    out_file.seek(0)
    sys.stdout.write(out_file.read().decode())
    sys.stdout.flush()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=1, help="timed regions of --steps steps, the median one reported (0: >= 25, until 1 s of them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the detection rows of the last timed step as DIR/<field>.npy (float64; rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="beyond the headline: live parity, per-kernel roofline, counters, lane overlap, the other configs, "
                         "host-frame / plugin legs, the other programs and the CPU baseline (the --no-* options trim these)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-legs", action="store_true", help="skip the other BASELINE configs / host-frame / plugin legs")
    ap.add_argument("--no-fp32-leg", action="store_true", help="skip the -p 32 and --plain-fp16 engine legs (profiling runs: one engine's kernels only)")
    ap.add_argument("--no-parity", action="store_true", help="skip the live score check against the oracle")
    ap.add_argument("--table", default=None, help="write the per-kernel roofline table (JSON) here")
    ap.add_argument("--no-live-pmc", action="store_true", help="take roofline.traffic from the committed profiles/pmc_traffic.json instead of two rocprofv3 --pmc passes of this run")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--schedule-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-numa", action="store_true", help="N > 1: do not pin the ranks to their GPUs' NUMA nodes")
    ap.add_argument("--fail-rank", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dry-run", action="store_true",
                    help="harness self-test without a GPU: a stub engine that sleeps 2 ms per step (used by the "
                         "world_size-2 tests; its output is marked invalid)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.table and not args.full:
        ap.error("--table is written by the roofline pass of --full")

    if args.pmc_child:
        return pmc_child()
    if args.schedule_child:
        return schedule_child()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))

    # libwatsor_hip.so owns the GPU side (its own HIP streams, events, graphs): load it FIRST so it binds
    # to /opt/rocm's HIP runtime, and never initialise torch's bundled copy of that runtime in this
    # process.  torch is used for its CPU side only: the rendezvous/barrier/max-over-ranks (gloo -- the
    # path has no data-path collective) and the oracle's conv2d in the parity / cpu_baseline legs.
    from watsor_amd import engine as builder
    from watsor_amd.synth import synthetic_frame, synthetic_weights
    if args.dry_run:
        HipEngine = _StubEngine
    else:
        from watsor_amd.runtime import HipEngine
        from watsor_amd import _lib
        _lib.load()
        note("library loaded")

    dist = None
    if world > 1:
        import torch
        import torch.distributed as dist
        import datetime
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=RANK_START_TIMEOUT_S))
        note("process group up (gloo)")

    numa_info = None
    if world > 1 and not args.dry_run and not args.no_numa:
        # one process per GPU on a two-socket host: run (and first-touch every page-locked block) on the GPU's own NUMA node
        from watsor_amd import numa
        numa_info = numa.pin_to_gpu_node(local_rank)
        note("rank %d: GPU %s on NUMA node %d, pinned to %d CPUs" % (rank, numa_info["pci"], numa_info["numa_node"], numa_info["cpus"]))
    if args.fail_rank is not None and rank == args.fail_rank:      # (harness self-test: a rank that dies before the rendezvous)
        sys.exit(3)

    model_dir = "/tmp/wz_bench_%d_%d" % (os.getpid(), rank)
    os.makedirs(model_dir, exist_ok=True)
    engine_path = os.path.join(model_dir, "mi355x.bin")
    if args.dry_run:
        weights = None
        open(engine_path, "wb").close()
    else:
        weights = synthetic_weights(1234)
        builder.save_engine(builder.build_engine(weights, **HEADLINE_PROGRAM), engine_path)     # the robust -p 16 program (HEADLINE_PROGRAM)

    note("engine file built")
    eng = HipEngine(engine_path, local_rank, BATCH, WIDTH, HEIGHT)
    note("engine created on " + eng.device_name)
    # camera `rank`: a ring of 5 batches of distinct frames, pre-staged in HBM.  Coprime with the lane count (4): a lane's frame
    # slots see a different scene every step, so the NMS kernel's per-slot band hint is never a replay of its last call
    ring = RING
    host_frames = [synthetic_frame(WIDTH, HEIGHT, 1234 + rank * 1000 + i) for i in range(ring * BATCH if not args.dry_run else 2)]
    if args.dry_run:
        host_frames = (host_frames * (ring * BATCH))[:ring * BATCH]
    d_frames = [eng.upload(f) for f in host_frames]
    ws, hs = [WIDTH] * BATCH, [HEIGHT] * BATCH

    lanes = eng.num_slots

    def submit(step):
        b = step % ring
        eng.submit_device(step % lanes, d_frames[b * BATCH:(b + 1) * BATCH], ws, hs)

    def barrier():
        # barrier + device synchronize on both sides of a timed region (eng.sync() = hipStreamSynchronize of every
        # stream this process ever enqueues GPU work on)
        eng.sync()
        if dist is not None:
            dist.barrier()

    note("frames staged in HBM")
    for s in range(args.warmup):
        submit(s)
    barrier()
    note("warm-up done")
    rounds = []
    spent = 0.0
    while True:
        barrier()
        t0 = time.perf_counter()
        for s in range(args.steps):
            submit(s)
        eng.sync()                            # device synchronize: this rank's K steps are done -> stop ITS clock here ...
        el = time.perf_counter() - t0
        if dist is not None:                  # ... then the barrier, outside the clock (a gloo barrier over TCP costs as much as a step)
            dist.barrier()
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        rounds.append(el)
        spent += el
        if args.rounds > 0:
            more = len(rounds) < args.rounds
        else:
            more = len(rounds) < (3 if args.dry_run else MIN_ROUNDS) or (not args.dry_run and spent < ROUNDS_BUDGET_S and len(rounds) < MAX_ROUNDS)
        if dist is not None:      # every rank runs the same number of rounds: rank 0 decides
            flag = torch.tensor([1 if more else 0])
            dist.broadcast(flag, 0)
            more = bool(flag.item())
        if not more:
            break
    elapsed = float(np.median(rounds))
    note("timed: %d rounds of %d steps, median %.4f s (min %.4f, max %.4f)" % (len(rounds), args.steps, elapsed, min(rounds), max(rounds)))
    if args.dump_outputs and rank == 0:
        # the last timed step ran on lane (steps - 1) % lanes; the loops below reuse that lane's rows
        dump_outputs(eng.slot_rows((args.steps - 1) % lanes, BATCH), args.dump_outputs)
        note("outputs of the last timed step written to %s" % args.dump_outputs)

    # per-step latency (synchronous steps), outside the timed regions
    lat = []
    for s in range(min(max(args.steps, 50), 100)):
        t1 = time.perf_counter()
        submit(s)
        eng.wait(s % lanes)
        lat.append((time.perf_counter() - t1) * 1e3)
    rows = eng.slot_rows((len(lat) - 1) % lanes, BATCH)
    detections_per_frame = float((rows["confidence"] > 0).sum()) / BATCH

    rank_legs = None
    if world > 1 and not args.dry_run and args.full and not args.no_legs:
        # every rank: its timed engine away first (one engine's streams at a time), then the host-side legs TOGETHER
        if rank != 0:
            eng.close()
    out = None
    frames_per_round = args.steps * BATCH * world
    if rank == 0 and args.dry_run:
        out = {"metric": "DRY RUN (stub engine, no GPU) -- invalid as a measurement",
               "value": round(frames_per_round / elapsed, 2), "unit": "frames/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
               "rounds": len(rounds), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "none",
               "data": "synthetic", "config": {"workload": "dry-run"},
               "camera_seeds": [1234 + r * 1000 for r in range(world)]}
    elif rank == 0:
        note("latency loop done")
        parity = None
        if args.full and not args.no_parity:
            parity = parity_leg(eng, host_frames, d_frames, weights)
            note("parity: max |dscore| %.6f, max |dbox| %d px over %d rows; %d rows without a partner (%d unexplained)"
                 % (parity["max_dscore"], parity["max_dbox_px"], parity["rows_compared"], parity["rows_without_partner"], parity["rows_unexplained"]))
        eng.submit_device(0, d_frames[:BATCH], ws, hs)
        eng.wait(0)
        graph_nodes = eng.graph_nodes(0)   # as captured: kernel launches (+ a descriptor copy where the resize kernel does not take them as arguments)
        input_size, hp_blocks = eng.input_size, eng.hp_blocks
        eng.close()                        # (one engine's streams at a time: eight live streams leave later engines sharing hardware queues)
        roof = None
        if args.full:
            # per-kernel durations: HIP events around every launch (wz_profile_stages) -- an entry point of the DEVELOPMENT library
            # (the same sources built with -DWZ_DEV_BUILD; the headline above was timed on libwatsor_hip.so, which has no such hooks)
            prof = HipEngine(engine_path, local_rank, BATCH, WIDTH, HEIGHT, dev=True)
            pd = [prof.upload(f) for f in host_frames[:BATCH]]
            ops = prof.ops()
            stages = prof.profile_device(pd, ws, hs, reps=10, inner=PROFILE_INNER)
            single = prof.profile_device(pd, ws, hs, reps=10, inner=1)
            prof.close()
            note("stage profiles done")
            table, overhead = aggregate_stages(stages, ops, BATCH, WIDTH * HEIGHT * 3, input_size, hp_blocks, PROFILE_INNER)
            single_table, _ = aggregate_stages(single, ops, BATCH, WIDTH * HEIGHT * 3, input_size, hp_blocks, 1)
            roof = roofline_object(table, overhead, single_table, PROFILE_INNER, robust=hp_blocks >= 17)
            if args.table:
                json.dump(dict(stages=stages, stages_single_bracket=single, inner=PROFILE_INNER, kernels=table,
                               kernels_single_bracket=single_table), open(args.table, "w"), indent=1)
        out = {
            "metric": "detected frames/sec (whole node) + p50 per-frame latency, SSD-MobileNet 300x300",
            "value": round(frames_per_round / elapsed, 2), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "rounds": len(rounds),
            "value_min": round(frames_per_round / max(rounds), 2), "value_max": round(frames_per_round / min(rounds), 2),
            "p50_ms": round(float(np.median(lat)), 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f16", "data": "synthetic",
            "config": {"workload": "1 synthetic 640x480 RGB stream per GPU, batch=8 frames, SSD-MobileNet-v2 300x300 "
                                   "(seeded random-init weights), frames resident in HBM, rows copied back to host",
                       "engine": ("-p 16 --robust (fp16 MFMA; all 17 blocks with split hi+lo operands, 16-bit float-form chunk buffer up to block 9, "
                                  "Conv_1 with split weights): the program built for trained, BatchNorm-folded weights") if hp_blocks == 17
                                 else "-p 16 (fp16 MFMA; stem + blocks 0..%d with split hi+lo operands, the rest plain fp16)" % (hp_blocks - 1)
                                 if hp_blocks else "-p 16 --plain-fp16",
                       "batch": BATCH, "frame": "%dx%d" % (WIDTH, HEIGHT), "parallelism": "replica-per-gpu x%d" % world, "batches_in_flight": lanes,
                       "graph_nodes_per_batch": graph_nodes, "detections_per_frame": detections_per_frame,
                       **({"n_gpus_note": "value = %d independent replicas, each on frames resident in its own HBM: linear by construction (no collective, no "
                                          "shared resource but the host); the shared-host measurement of an N > 1 run is legs_all_ranks_concurrently (--full) "
                                          "(page-locked host frames, every rank at the same time)" % world} if world > 1 else {})},
        }
        if args.full:
            out["parity"] = parity
            out["roofline"] = roof
        if world == 1 and args.full and not args.no_live_pmc:
            live = live_pmc_traffic()
            note("live counter passes %s" % ("done" if live else "unavailable (committed json kept)"))
            if live and roof["kernel"] in live:
                roof["traffic"] = live[roof["kernel"]]
                roof["frac_counter_traffic"] = round(roof["traffic"]["bytes"] / (roof["avg_launch_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 5)
                roof["traffic_over_fused_min"] = round(roof["traffic"]["bytes"] / max(roof["fused_min_bytes_per_launch"], 1), 3)
                out["roofline"] = roof
        if world == 1 and args.full and not args.no_live_pmc:
            lo = lane_overlap()
            note("lane overlap %s" % ("measured" if lo and lo["source"].startswith("live") else "from the committed file" if lo else "unavailable"))
            if lo:
                # what the four-lane headline rests on: how many kernels are on the chip at once, and what they book of it
                out["roofline"]["concurrency_mean"] = lo["kernels_in_flight_mean_while_busy"]
                out["roofline"]["cu_slot_time_us_per_step"] = lo["cu_slot_time_us_per_step"]
                out["roofline"]["lane_overlap"] = lo
        if world == 1 and args.full and not args.no_legs:
            legs = {}
            legs.update(host_legs(engine_path, model_dir, local_rank, host_frames))
            note("host-frame legs done")
            legs.update(config_legs(engine_path, local_rank, rank, weights))
            note("config legs done")
            legs.update(host_config_legs(engine_path, local_rank))
            note("host-memory config legs done")
            legs["busy_scene_b8"] = busy_scene_leg(host_frames, rank)
            note("busy-scene leg done")
            legs["latency_schedule_b8"] = latency_schedule_leg()
            note("latency-schedule leg done")
            legs.update(worker_legs(model_dir))
            note("worker legs done")
            out["legs"] = legs
        if world == 1 and args.full and not args.no_fp32_leg:
            out["default_program_engine"] = default_program_leg(weights, host_frames, rank)
            try:     # the dominant kernel of THAT program under the same rule (13 launches of wz_k_mbconv_hp: the large and the 19x19 maps only)
                builder.save_engine(builder.build_engine(weights), engine_path)
                prof = HipEngine(engine_path, local_rank, BATCH, WIDTH, HEIGHT, dev=True)
                pd = [prof.upload(f) for f in host_frames[:BATCH]]
                st = prof.profile_device(pd, ws, hs, reps=10, inner=PROFILE_INNER)
                tb, ov = aggregate_stages(st, prof.ops(), BATCH, WIDTH * HEIGHT * 3, prof.input_size, prof.hp_blocks, PROFILE_INNER)
                prof.close()
                r2 = roofline_object(tb, ov, [], PROFILE_INNER)
                out["default_program_engine"]["roofline"] = {k: r2[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_us",
                                                                                 "launches_per_step", "algorithmic_bytes_per_launch") if k in r2}
                if "arithmetic_free_skeleton" in r2:
                    out["default_program_engine"]["roofline"]["frac_if_arithmetic_were_free"] = r2["frac_if_arithmetic_were_free"]
            except Exception as e:
                out["default_program_engine"]["roofline"] = dict(error=repr(e))
            out["plain_fp16_engine"] = plain_fp16_leg(weights, host_frames, rank)
            out["fp32_engine"] = fp32_engine_leg(weights, host_frames, rank)
            note("other-precision legs done")
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(weights, host_frames[:BATCH])
            note("cpu baseline done")
    if world > 1 and args.full and not args.no_legs:
        stub = [("stub", lambda: {"host_frames_pinned_b8": dict(value=1000.0 + rank, p50_ms=1.0, workload="dry-run stub")})] if args.dry_run else None
        gathered = all_rank_legs(engine_path, model_dir, local_rank, host_frames, dist, world, plan=stub,
                                 rank_info=numa_info or dict(device=local_rank, numa_node=-1, pinned=False))
        if out is not None:
            out["legs_all_ranks_concurrently"] = summarise_rank_legs(gathered)
            note("host-side legs on all ranks done")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if out is not None:
        if world > 1 and args.full:
            out["only_at_n_gpus_1"] = "cpu_baseline, live counter traffic, lane overlap, the other-engine legs and the single-process legs run at N = 1 only"
        print(json.dumps(out), flush=True)
    try:
        os.remove(engine_path)
        os.rmdir(model_dir)
    except OSError:
        pass


if __name__ == "__main__":
    main()

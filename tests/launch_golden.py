"""What the network enqueue (watsor_amd/csrc/wz_network.hip) launches, pinned: for every engine program, environment and batch size
of the tables below, the launches of one batch -- (kernel name, workgroups, threads, LDS bytes) in order, as the measurement library
(`make stamps`) notes them --, the nodes of the captured graph, the two flags of the post-processing (boxes decoded by the grouped
reduce, candidates listed by it), the names of the profile's stages and the SHA-256 of the rows written for fixed frames.
tests/golden/network_launches.json holds the recording (tests/golden/make_network_launches_golden.py writes it),
tests/test_gpu_network_launches.py compares.

The knobs are read when an engine is created and some of them once per process: one child process per environment, started one
after the other, each under its own time limit.

    python tests/launch_golden.py --child <environment> <models.json> <out.json> <program> [<program> ...]
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PATH = os.path.join(HERE, "golden", "network_launches.json")
STAMPS = os.path.join(ROOT, "watsor_amd", "libwatsor_hip_stamps.so")

MAX_BATCH = 8
BATCHES = (1, 2, 3, 8)                    # 1 .. 3: the small-batch launch shapes; 8: the headline
FRAME_SEED = 4200

# program -> (weights of watsor_amd.synth, build_engine's arguments)
PROGRAMS = {
    "default": ("synthetic_weights", {}),
    "robust": ("synthetic_weights", dict(robust=True)),
    "plain": ("synthetic_weights", dict(hp_upto=-1)),
    "unfused": ("synthetic_weights", dict(fuse=False)),
    "stem_separate": ("synthetic_weights", dict(fuse_stem=False)),
    "fp32": ("synthetic_weights", dict(precision=32)),
    "inception_v2": ("synthetic_inception_v2", dict(precision=16)),
    "mobilenet_v1": ("synthetic_mobilenet_v1", dict(precision=16, fuse=True)),
    # No program of the builder has more head ops than the grouped reduce takes (six [box | class] heads against WZ_REDUCE_GROUP_MAX 8):
    # the default program with every head op listed twice has twelve.  Listed as h0 h0 h1 h1 h2 h2 h3 h4 h5 h3 h4 h5: the first six
    # fill the wide head kernel's launch (each pair with the same K slices: two entries of the grouped reduce that store the same
    # values), h3 and h4 take the reduce's last two entries by another route, and the last four are refused a parking slab -- they
    # reduce on their own, earlier in the stream, so the boxes are NOT all finished by the grouped reduce (decode_fused false).
    "heads_twice": ("synthetic_weights", dict(heads_twice=True)),
}


def heads_twice(image):
    """The engine image with each of its six head ops (out_mode != 0, the last ops) listed twice, in the order PROGRAMS explains."""
    import struct
    from watsor_amd.engine import OP_RECORD_BYTES, _align
    h = list(struct.unpack_from("<10I6f6Q12I", image))
    n_ops, ops_off, anchors_off, weights_off, weights_bytes = h[7], h[17], h[18], h[19], h[20]
    ops = [image[ops_off + OP_RECORD_BYTES * i:ops_off + OP_RECORD_BYTES * (i + 1)] for i in range(n_ops)]
    heads = [r for r in ops if struct.unpack_from("<i", r, 15 * 4)[0] != 0]
    assert len(heads) == 6 and ops[-6:] == heads
    ops = ops[:-6] + [heads[k] for k in (0, 0, 1, 1, 2, 2, 3, 4, 5, 3, 4, 5)]
    anchors = image[anchors_off:weights_off]
    h[7], h[18] = len(ops), _align(ops_off + OP_RECORD_BYTES * len(ops))
    h[19] = h[18] + len(anchors)
    h[21] = h[19] + weights_bytes
    return b"".join([struct.pack("<10I6f6Q12I", *h), image[160:ops_off], b"".join(ops), bytes(h[18] - ops_off - OP_RECORD_BYTES * len(ops)),
                     anchors, image[weights_off:weights_off + weights_bytes]])


# environment -> (variables, programs, batch sizes).  WZ_GRAPH=1: the batch is captured (`lone` false); 0: kernel by kernel (`lone` true,
# which changes what the block launchers choose).
KNOB_PROGRAMS = ("default", "robust")
ENVIRONMENTS = {
    "graph": (dict(WZ_GRAPH="1"), tuple(PROGRAMS), BATCHES),
    "kernel_by_kernel": (dict(WZ_GRAPH="0"), tuple(PROGRAMS), BATCHES),
    "no_splitk": (dict(WZ_GRAPH="1", WZ_SPLITK="0"), KNOB_PROGRAMS, (8,)),
    "heads_not_deferred": (dict(WZ_GRAPH="1", WZ_DEFER_HEADS="0", WZ_CONV_WIDE="0"), KNOB_PROGRAMS, (8,)),
    "no_conv_wide": (dict(WZ_GRAPH="1", WZ_CONV_WIDE="0"), KNOB_PROGRAMS, (8,)),
    "decode_not_fused": (dict(WZ_GRAPH="1", WZ_FUSE_DECODE="0"), KNOB_PROGRAMS, (8,)),
    "no_extras_pair": (dict(WZ_GRAPH="1", WZ_EXTRAS_PAIR="0"), KNOB_PROGRAMS, (8,)),
}
CASES = [(program, env) for env, (_, programs, _) in ENVIRONMENTS.items() for program in programs]
KNOBS = sorted({k for variables, _, _ in ENVIRONMENTS.values() for k in variables} | {"WZ_SCHEDULE", "WZ_LANES", "WZ_STREAMS"})


def build_models(directory):
    """One engine file per program under `directory`; returns {program: path of its mi355x.bin}."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from watsor_amd import engine, synth
    weights, out = {}, {}
    for program, (source, kw) in PROGRAMS.items():
        if source not in weights:
            weights[source] = getattr(synth, source)(1234)
        d = os.path.join(str(directory), program)
        os.makedirs(d, exist_ok=True)
        out[program] = os.path.join(d, "mi355x.bin")
        kw = dict(kw)
        twice = kw.pop("heads_twice", False)
        image = engine.build_engine(weights[source], **kw)
        engine.save_engine(heads_twice(image) if twice else image, out[program])
    return out


def record(case, models):
    """The recording of case (program, environment), in a process whose environment already is that environment's and whose
    development library is the measurement build: {"stages": [...], "batches": {n: {launches, graph_nodes, decode_fused,
    cands_listed, rows_sha256}}}."""
    import numpy as np
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from watsor_amd.runtime import ROW_DTYPE, HipEngine
    from watsor_amd.synth import synthetic_frame
    program, env = case
    frames = [synthetic_frame(640, 480, FRAME_SEED + i) for i in range(MAX_BATCH)]
    e = HipEngine(models[program], 0, MAX_BATCH, 640, 480, dev=True)
    try:
        out = dict(stages=e.stage_names(), batches={})
        for n in ENVIRONMENTS[env][2]:
            rows = [np.zeros(100, ROW_DTYPE) for _ in range(n)]
            e.detect_batch(frames[:n], rows)
            name, dims, flags = C.create_string_buffer(512), (C.c_int32 * 8)(), (C.c_int32 * 2)()
            count = e._lib.wz_debug_lane_launch(e._h, 0, 0, name, 512, dims)
            assert count > 0, "no launch notes: is WATSOR_HIP_DEV_LIBRARY the measurement build?"
            launches = []
            for i in range(count):
                assert e._lib.wz_debug_lane_launch(e._h, 0, i, name, 512, dims) == count
                launches.append([name.value.decode(), int(dims[0]), int(dims[1]), int(dims[2])])
            null = C.c_void_p(None)
            e._ck(e._lib.wz_debug_post_lane(e._h, 0, n, null, null, null, null, null, null, null, C.byref(flags)))
            out["batches"][str(n)] = dict(launches=launches, graph_nodes=e.graph_nodes(0), decode_fused=bool(flags[0]),
                                          cands_listed=bool(flags[1]), rows_sha256=hashlib.sha256(np.stack(rows).tobytes()).hexdigest())
        return out
    finally:
        e.close()


def run_child(env, programs, models_json, out_json, timeout):
    """A fresh process with environment `env` records `programs` into `out_json`; returns the CompletedProcess."""
    variables = {k: v for k, v in os.environ.items() if k not in KNOBS}
    variables.update(ENVIRONMENTS[env][0], WATSOR_HIP_DEV_LIBRARY=STAMPS)
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env, models_json, out_json] + list(programs),
                          env=variables, capture_output=True, text=True, timeout=timeout)


def write_golden(cases):
    """{case key: recording} -> PATH; the file names every kernel once (`kernels`), its launches carry the index."""
    kernels = sorted({l[0] for c in cases.values() for b in c["batches"].values() for l in b["launches"]})
    index = {k: i for i, k in enumerate(kernels)}
    for c in cases.values():
        for b in c["batches"].values():
            b["launches"] = [[index[l[0]]] + l[1:] for l in b["launches"]]
    with open(PATH, "w") as f:
        json.dump(dict(kernels=kernels, cases=cases), f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


def golden():
    """{case key: recording}, the launches with their kernels' names again"""
    with open(PATH) as f:
        g = json.load(f)
    for c in g["cases"].values():
        for b in c["batches"].values():
            b["launches"] = [[g["kernels"][l[0]]] + l[1:] for l in b["launches"]]
    return g["cases"]


def key(case):
    return "%s/%s" % case


if __name__ == "__main__":
    if len(sys.argv) < 6 or sys.argv[1] != "--child":
        sys.exit(__doc__)
    env, models_json, out_json = sys.argv[2:5]
    with open(models_json) as f:
        models = json.load(f)
    with open(out_json, "w") as f:
        json.dump({key((p, env)): record((p, env), models) for p in sys.argv[5:]}, f)

"""Batches as production runs them -- detect_batch / submit_host + collect on an engine larger than the batch, the resize kernel's own
input tensor (a pair input with its lo half), captured graph or kernel by kernel with `lone` set, buffers shared, any lane, after
other batches -- for tests/test_gpu_production_walk.py (the op-by-op walk of op_reference on what such a batch left in lane 0's
tensors) and tests/test_gpu_production_bits.py (head outputs bit for bit: shared buffers against kept ones, every lane, after a
poisoned batch and after batches of other sizes).

WZ_GRAPH is the knob that decides `lone`; knobs are read when an engine is created and some of them once per process: nothing here
runs in the test's own process.  The bit comparison starts one child per (program, environment) (`run_child`); the walk, whose
children would each spend most of their time on imports, one per environment that takes the cases one after the other, each under
its own time limit (`Worker`).

    python tests/production_batches.py <job.json> <out.json>        (job: {"mode": "walk" | "bits", "program": ..., ...})
    python tests/production_batches.py --serve                      (jobs on stdin, one line of JSON each)
"""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SEED = 1234
MAX_BATCH = 9                     # larger than every batch of the walk; the poisoning pass and one batch of the sequence fill it
MAX_W, MAX_H = 1280, 720
FRAME_SEED = 7300

ENVIRONMENTS = {"graph": dict(WZ_GRAPH="1"), "kernel_by_kernel": dict(WZ_GRAPH="0")}
KNOBS = ("WZ_GRAPH", "WZ_SCHEDULE", "WZ_LANES", "WZ_STREAMS", "WZ_NO_BUFFER_REUSE")

# ---------------------------------------------------------------------------------------------------------------------------------
# the walk's programs: name -> (weights of watsor_amd.synth, precision, build_engine's arguments, fused blocks, last float-form block,
#                               case key of tests/golden/network_launches.json that records its post-processing flags or None)
# ---------------------------------------------------------------------------------------------------------------------------------
WALK_PROGRAMS = {
    "default":          ("synthetic_weights", 16, dict(), 17, -1, "default"),
    "robust":           ("synthetic_weights", 16, dict(robust=True), 17, 9, "robust"),
    "stem_separate":    ("synthetic_weights", 16, dict(fuse_stem=False), 17, -1, "stem_separate"),
    "mobilenet_v2_p32": ("synthetic_weights", 32, dict(), 0, -1, "fp32"),
    "inception_v2_p32": ("synthetic_inception_v2", 32, dict(), 0, -1, None),
    "mobilenet_v1_p32": ("synthetic_mobilenet_v1", 32, dict(), 0, -1, None),
    "inception_v2_p16": ("synthetic_inception_v2", 16, dict(), 0, -1, "inception_v2"),
    "mobilenet_v1_p16": ("synthetic_mobilenet_v1", 16, dict(fuse=True), 0, -1, "mobilenet_v1"),
}
# (program, environment, batch size).  kernel_by_kernel: WzMbArgs::lone is set -- launch A of blocks 13 .. 16
# (robust program) takes the two-waves-per-chunk form up to 128 workgroups: block 13 at n = 3 .. 5, blocks 14 .. 16 at n = 5 .. 8.
WALK_CASES = [(p, env, n) for p, env, ns in (
    ("default", "kernel_by_kernel", (3, 5, 8)), ("robust", "kernel_by_kernel", (3, 5, 8)),
    ("default", "graph", (3,)), ("robust", "graph", (3,)),
    ("stem_separate", "graph", (2,)),
    ("mobilenet_v2_p32", "graph", (1, 3)), ("inception_v2_p32", "graph", (1, 3)), ("mobilenet_v1_p32", "graph", (1, 3)),
    ("inception_v2_p16", "graph", (3,)), ("mobilenet_v1_p16", "graph", (3,)),
) for n in ns]
PAIR_INPUT = ("default", "robust", "mobilenet_v2_p32", "inception_v2_p32", "mobilenet_v1_p32")
LO_POPULATED = 0.90               # of a frame's R, G, B elements (oracle.preprocess alone: 95.5 % at 300x300, 99.8 % at 640x480, 1280x720)

# the bit comparison's batch sizes and lanes, in order
SEQUENCE = ((8, 0), (3, 1), (9, 2), (1, 3), (5, 0), (2, 1), (6, 2))


def arch_program(name):
    """The arch.Program that build_engine packs for WALK_PROGRAMS[name]"""
    from watsor_amd import arch, inception, mobilenet_v1
    return {
        "default": lambda: arch.build(hp_upto=arch.HP_LAST_BLOCK),
        "robust": lambda: arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True),
        "stem_separate": lambda: arch.build(fuse_stem=False),
        "mobilenet_v2_p32": lambda: arch.build(fuse=False, input_pair=True),
        "inception_v2_p32": lambda: inception.build(input_pair=True),
        "mobilenet_v1_p32": lambda: mobilenet_v1.build(fuse=False, input_pair=True),
        "inception_v2_p16": lambda: inception.build(),
        "mobilenet_v1_p16": lambda: mobilenet_v1.build(fuse=True),
    }[name]()


def walk_frames(n, pair):
    """n frames of mixed sizes, no two alike: synthetic 640x480, synthetic 1280x720, synthetic 300x300 (the resize copies), uniform
    noise 640x480, one constant frame -- for a pair input a second synthetic 1280x720 in its place (a constant frame's lo half is one
    value: nothing for the population condition to count) --, then synthetic ones of the three sizes again."""
    from watsor_amd.synth import synthetic_frame
    rng = np.random.Generator(np.random.PCG64(FRAME_SEED))
    sizes = ((640, 480), (1280, 720), (300, 300))
    out = []
    for i in range(n):
        if i == 3:
            out.append(rng.integers(0, 256, (480, 640, 3), dtype=np.uint8))
        elif i == 4 and not pair:
            out.append(np.full((480, 640, 3), (37, 142, 219), np.uint8))
        else:
            w, h = sizes[1] if i == 4 else sizes[i % 3]
            out.append(synthetic_frame(w, h, FRAME_SEED + i))
    return out


def stored_input(frame, size, pair):
    """What the resize kernel must store for `frame`: (hi, lo) float16 [size,size,4], channel 3 zero; lo None for a plain input."""
    from oracle import preprocess as pre
    v = pre.preprocess(frame, size)
    hi = np.zeros((size, size, 4), np.float16)
    hi[..., :3] = v.astype(np.float16)
    if not pair:
        return hi, None
    lo = np.zeros((size, size, 4), np.float16)
    lo[..., :3] = (v - hi[..., :3].astype(np.float32)).astype(np.float16)
    return hi, lo


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _engine(path, keep):
    from watsor_amd.runtime import HipEngine
    if keep:
        os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        return HipEngine(path, 0, MAX_BATCH, MAX_W, MAX_H, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE", None)


def _rows(n):
    from watsor_amd.runtime import ROW_DTYPE
    return [np.zeros(100, ROW_DTYPE) for _ in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# child: the walk
# ---------------------------------------------------------------------------------------------------------------------------------
_weights = {}                     # (a worker's jobs share them)


def child_walk(job):
    import op_reference as R
    from watsor_amd import arch, engine, synth
    name = job["program"]
    source, precision, kw, n_blocks, float_form_upto, _ = WALK_PROGRAMS[name]
    if source not in _weights:
        _weights[source] = getattr(synth, source)(SEED)
    weights = _weights[source]
    prog = arch_program(name)
    pair = bool(prog.tensors["input"].hp)
    path = os.path.join(job["dir"], "mi355x.bin")
    engine.save_engine(engine.build_engine(weights, precision, **kw), path)
    e = _engine(path, keep=True)
    out = dict(input_pair=pair, ops=len(prog.ops), blocks=sum(op.kind == arch.OP_MBCONV for op in prog.ops), batches={})
    try:
        assert e.tensors()[0][0] == "input" and e.tensor_is_pair(0) == pair and e.precision == precision
        assert {t[0] for t in e.tensors()} == {"input"} | {t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t}
        assert len(e.ops()) == len(prog.ops)
        for n in job["batches"]:
            t0 = time.time()
            frames = walk_frames(n, pair)
            e.detect_batch(frames, _rows(n))
            post = e.stage_post_lane(0, n)
            b = dict(graph_nodes=e.graph_nodes(0), decode_fused=post["decode_fused"], cands_listed=post["cands_listed"],
                     sizes=["%dx%d" % (f.shape[1], f.shape[0]) for f in frames], input_differs=[], lo_populated=[])
            for i, f in enumerate(frames):                   # the resize inside a batch, frame by frame, bit for bit
                hi, lo = stored_input(f, prog.size, pair)
                ghi, glo = e.stage_read_tensor(0, i, halves=True)
                bad = int((_bits(ghi) != _bits(hi)).sum()) + (int((_bits(glo) != _bits(lo)).sum()) if pair else 0)
                if bad or (glo is None) != (lo is None):
                    b["input_differs"].append("frame %d (%s): %d halves differ from oracle.preprocess" % (i, b["sizes"][i], bad))
                if pair:
                    b["lo_populated"].append(float((glo[..., :3] != 0).mean()))
            t1 = time.time()
            rep = R.walk(e, prog, weights, None, precision, frames=R.frame_subset(n, 3 if n_blocks else 8), check=False,
                         float_form_upto=float_form_upto, heads=(post["box_enc"], post["logits"]))
            b.update(failures=rep.failures[:20], n_failures=len(rep.failures), summary=rep.summary(), ops_checked=rep.ops_checked,
                     blocks_checked=rep.blocks_checked, ops_unchecked=rep.ops_unchecked, ops_mbconv=rep.ops_mbconv, elements=rep.elements,
                     worst=max(v[0] for v in rep.worst.values()) if rep.worst else None,
                     seconds_batch=round(t1 - t0, 2), seconds_walk=round(time.time() - t1, 2))
            out["batches"][str(n)] = b
    finally:
        e.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# child: bits
# ---------------------------------------------------------------------------------------------------------------------------------
def bits_frames():
    """MAX_BATCH + len(SEQUENCE) different 640x480 frames: batch j of the sequence takes frames j .. j + n - 1, so no two batches
    start with the same frame."""
    from watsor_amd.synth import synthetic_frame
    return [synthetic_frame(640, 480, FRAME_SEED + 100 + i) for i in range(MAX_BATCH + len(SEQUENCE))]


def _poison(e):
    """Lane 0's tensors, slots and workspace full of NaN: the network at the engine's largest batch on an all-NaN input."""
    from hp_halo_gather import NAN_PATTERNS
    S = e.input_size
    x = np.resize(np.array(NAN_PATTERNS, np.uint16), MAX_BATCH * S * S * 4).view(np.float16).reshape(MAX_BATCH, S, S, 4)
    assert np.isnan(x).all()
    be, lg = e.stage_forward(x)
    return float(np.isnan(lg).mean())


def _heads(post):
    return _bits(post["box_enc"]), _bits(post["logits"])


def child_bits(job):
    import launch_golden
    from watsor_amd import engine, synth
    name = job["program"]
    source, kw = launch_golden.PROGRAMS[name]
    path = os.path.join(job["dir"], "mi355x.bin")
    packed, assign = [], engine.assign_slots
    engine.assign_slots = lambda prog, names: packed.append(assign(prog, names)) or packed[-1]
    try:
        engine.save_engine(engine.build_engine(getattr(synth, source)(SEED), **kw), path)
    finally:
        engine.assign_slots = assign
    frames = bits_frames()
    kept, shared = _engine(path, keep=True), _engine(path, keep=False)
    out = dict(batches=[], four_lanes=[], messages=[])
    try:
        assert len(packed) == 1 and len(packed[0]) == len(kept.tensors()) == len(shared.tensors())
        out["slots"] = [max(packed[0]) + 1, len(packed[0])]         # buffers of the shared engine's lanes / of the kept engine's
        out["poison_nan"] = [_poison(kept), _poison(shared)]
        want = []
        for j, (n, lane) in enumerate(SEQUENCE):             # the kept engine: detect_batch, twice
            fr = frames[j:j + n]
            passes = []
            for _ in range(2):
                kept.detect_batch(fr, _rows(n))
                passes.append(_heads(kept.stage_post_lane(0, n)))
            want.append(passes[0])
            be, lg = passes[0]
            b = dict(n=n, lane=lane, kept_repeats=bool((passes[0][0] == passes[1][0]).all() and (passes[0][1] == passes[1][1]).all()),
                     finite=bool(np.isfinite(be.view(np.float32)).all() and np.isfinite(lg.view(np.float32)).all()),
                     frames_differ=all((lg[a] != lg[c]).any() for a in range(n) for c in range(a + 1, n)),
                     sha256=hashlib.sha256(be.tobytes() + lg.tobytes()).hexdigest(), kept_graph_nodes=kept.graph_nodes(0))
            out["batches"].append(b)
        firsts = [w[1][0].tobytes() for w in want]
        out["batches_differ"] = len(set(firsts)) == len(firsts)

        def compare(j, what):
            n, lane = SEQUENCE[j]
            be, lg = _heads(shared.stage_post_lane(lane, n))
            d = int((be != want[j][0]).sum()) + int((lg != want[j][1]).sum())
            if d:
                f = sorted(set(np.nonzero((lg != want[j][1]).reshape(n, -1).any(axis=1) | (be != want[j][0]).reshape(n, -1).any(axis=1))[0].tolist()))
                out["messages"].append("%s: batch %d of %d frames on lane %d: %d words of the head outputs differ from the kept engine's, "
                                       "frames %s" % (what, j, n, lane, d, f))
            return d == 0

        # all four lanes in flight before the first collect (the environment decides: captured graphs under WZ_GRAPH=1)
        rows = [_rows(SEQUENCE[j][0]) for j in range(4)]
        for j in range(4):
            shared.submit_host(SEQUENCE[j][1], frames[j:j + SEQUENCE[j][0]])
        for j in range(4):
            shared.collect(SEQUENCE[j][1], rows[j])
        for j in range(4):
            out["four_lanes"].append(dict(n=SEQUENCE[j][0], lane=SEQUENCE[j][1], equal=compare(j, "four lanes in flight"),
                                          graph_nodes=shared.graph_nodes(SEQUENCE[j][1])))
        # ... and the sequence, one batch at a time, each behind what the batches before it left
        for j, (n, lane) in enumerate(SEQUENCE):
            r = _rows(n)
            shared.submit_host(lane, frames[j:j + n])
            shared.collect(lane, r)
            out["batches"][j].update(shared_equals_kept=compare(j, "sequence"), shared_graph_nodes=shared.graph_nodes(lane))
    finally:
        shared.close()
        kept.close()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# parent
# ---------------------------------------------------------------------------------------------------------------------------------
def run_child(job, env, directory, timeout):
    """A fresh process with environment `env` (a key of ENVIRONMENTS) runs `job`; -> (CompletedProcess, the child's result or None)."""
    directory = str(directory)
    job = dict(job, dir=directory)
    job_json, out_json = os.path.join(directory, "job.json"), os.path.join(directory, "out.json")
    with open(job_json, "w") as f:
        json.dump(job, f)
    variables = {k: v for k, v in os.environ.items() if k not in KNOBS}
    variables.update(ENVIRONMENTS[env])
    p = subprocess.run([sys.executable, os.path.abspath(__file__), job_json, out_json], env=variables, capture_output=True, text=True,
                       timeout=timeout)
    if p.returncode != 0 or not os.path.isfile(out_json):
        return p, None
    with open(out_json) as f:
        return p, json.load(f)


class Worker:
    """A child process with environment `env` that takes jobs one after the other -- a line of JSON in, a line out -- each under its
    own time limit.  It pays for its start (the imports, HIP) once; every job creates and closes its own engine.  After a job that
    raised, ran out of time or took the process down the worker is gone for good: its later jobs fail at once, nothing is started
    again in that environment."""
    MARK = "RESULT "

    def __init__(self, env, directory):
        variables = {k: v for k, v in os.environ.items() if k not in KNOBS}
        variables.update(ENVIRONMENTS[env])
        self.env, self.gone = env, None
        self.log = open(os.path.join(str(directory), "worker_%s.log" % env), "w+")
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve"], env=variables, stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, stderr=self.log, text=True, bufsize=1)

    def _give_up(self, why):
        try:
            self.p.wait(timeout=5)                              # (it ends by itself after a job that raised)
        except subprocess.TimeoutExpired:
            self.p.kill()
            self.p.wait()
        self.log.seek(0)
        self.gone = "%s; the end of its stderr:\n%s" % (why, self.log.read()[-3000:])
        raise AssertionError("the %s child: %s" % (self.env, self.gone))

    def run(self, job, directory, timeout):
        import select
        assert self.gone is None, "the %s child is gone since an earlier job: %s" % (self.env, self.gone)
        try:
            self.p.stdin.write(json.dumps(dict(job, dir=str(directory))) + "\n")
            self.p.stdin.flush()
        except OSError as e:
            self._give_up("could not be given the job (%s)" % e)
        end = time.time() + timeout
        while True:
            ready, _, _ = select.select([self.p.stdout], [], [], max(0.0, end - time.time()))
            if not ready:
                self._give_up("no answer within %d s" % timeout)
            line = self.p.stdout.readline()
            if not line:
                self._give_up("ended with exit status %s" % self.p.wait())
            if line.startswith(self.MARK):
                out = json.loads(line[len(self.MARK):])
                if "error" in out:
                    self._give_up("the job raised:\n" + out["error"])
                return out

    def close(self):
        if self.p.poll() is None:
            try:
                self.p.stdin.close()
                self.p.wait(timeout=20)
            except (OSError, subprocess.TimeoutExpired):
                self.p.kill()
                self.p.wait()
        self.log.close()


def serve():
    """The worker's side: one job per line of stdin; the first job that raises is answered and ends the process."""
    import traceback
    for line in sys.stdin:
        job = json.loads(line)
        try:
            out = {"walk": child_walk, "bits": child_bits}[job["mode"]](job)
        except BaseException:
            out = dict(error=traceback.format_exc()[-4000:])
        sys.stdout.write(Worker.MARK + json.dumps(out) + "\n")
        sys.stdout.flush()
        if "error" in out:
            return 1
    return 0


if __name__ == "__main__":
    if len(sys.argv) not in (2, 3) or (len(sys.argv) == 2 and sys.argv[1] != "--serve"):
        sys.exit(__doc__)
    for d in (ROOT, HERE):
        if d not in sys.path:
            sys.path.insert(0, d)
    if len(sys.argv) == 2:
        sys.exit(serve())
    with open(sys.argv[1]) as f:
        job = json.load(f)
    result = {"walk": child_walk, "bits": child_bits}[job["mode"]](job)
    with open(sys.argv[2], "w") as f:
        json.dump(result, f)

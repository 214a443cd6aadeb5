"""Conv_1 on the dense 1x1 GEMM kernel (csrc/k_gemm_1x1.hip), checked on its own: the op's float64 reference on the source tensor the
engine itself stored (tests/op_reference.py: `reference`, `_compare` -- the bound of a plain conv, derived from the number formats: r
fp32 roundings over T, one fp16 store), through the development engine's product path (stage_forward, stage_read_tensor).

Reference anchor: Conv_1 is a layer inside `sess.run` of watsor/detection/tensorflow_cpu.py:113-115; there is no reference kernel.

Robust program: block 16 stores its fp16 output twice per pixel ([x | x], 640 channels) and Conv_1's weights are [hi | lo] along K = 640;
the kernel reads the first copy and multiplies it with both weight halves, so the reference is W_hi x + W_lo x on the read-back tensor and
the two copies must be bit-equal -- asserted here, it is the precondition of reading one.  Default program: K = 320, the plain form.
Batches: 8 (800 pixels: whole 32-pixel tiles; half of a 64-pixel one), 7 (700: the last tile holds 28 of 32 rows, the others read zeros
past the tensor's end), the smallest batch that takes the kernel (WZ_G1_MIN_M of the source) and the one below it (the older kernel: same
bound, nothing else asserted).
Frame independence: an output's K order depends on nothing but its channel tile, so a frame's Conv_1 tensor is the same bytes wherever the
frame sits in a batch and whatever the batch's size.  The extras' first 1x1 (K = 1 280) is not routed to this kernel: no case for it."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import conftest
import op_reference as R
import parity_utils as pu
from watsor_amd import arch
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

PROGRAMS = {"robust": lambda: arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True),
            "default": lambda: arch.build(hp_upto=arch.HP_LAST_BLOCK)}
PIXELS = 100                                        # Conv_1's map is 10 x 10


def _min_m():
    src = open(os.path.join(conftest.ROOT, "watsor_amd", "csrc", "k_gemm_1x1.hip")).read()
    return int(re.search(r"#define\s+WZ_G1_MIN_M\s+(\d+)", src).group(1))


FIRST_BATCH = max(1, -(-_min_m() // PIXELS))        # the smallest batch whose pixel count reaches the threshold


def _frame_input(seed):
    return pu.oracle_input_half([synthetic_frame(640, 480, 9000 + seed)])[0]


_inputs = {}


def _batch(n):
    """[n,S,S,4] float16: frames 0 .. n-1 of ONE eight-frame conformance batch (synthetic frame, noise, impulses, zeros, ...), so that
    frame f is the same input at every batch size."""
    if "x" not in _inputs:
        _inputs["x"] = R.conformance_batch(8, PROGRAMS["robust"]().size, 0, 77, _frame_input)
    return _inputs["x"][:n]


def _conv1(model_dir, x_half):
    """One forward pass on a buffer-keeping development engine -> (Conv_1's source [n,10,10,cin], Conv_1 [n,10,10,1280]) as stored."""
    os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        e = conftest.make_engine(model_dir, max_batch=8, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE")
    try:
        n = x_half.shape[0]
        e.stage_forward(x_half)
        idx = {name: i for i, (name, h, w, c) in enumerate(e.tensors())}
        src = np.stack([e.stage_read_tensor(idx["expanded_conv_16/output"], f) for f in range(n)])
        dst = np.stack([e.stage_read_tensor(idx["Conv_1"], f) for f in range(n)])
        return src, dst
    finally:
        e.close()


@pytest.fixture(scope="module")
def runs(model_dir_robust, model_dir_default):
    """(program, batch, reversed) -> (source, Conv_1), computed once and shared, never modified."""
    dirs = {"robust": model_dir_robust, "default": model_dir_default}
    cache = {}

    def get(program, n, reverse=False):
        key = (program, n, reverse)
        if key not in cache:
            x = _batch(n)
            src, dst = _conv1(dirs[program], x[::-1] if reverse else x)
            src.setflags(write=False)
            dst.setflags(write=False)
            cache[key] = (src, dst)
        return cache[key]
    yield get
    cache.clear()
    _inputs.clear()


def _check(program, synth_weights, src, dst):
    prog = PROGRAMS[program]()
    idx, op = next((i, o) for i, o in enumerate(prog.ops) if o.kind == arch.OP_CONV and o.dst == "Conv_1")
    n = src.shape[0]
    assert dst.shape == (n, 10, 10, 1280) and src.shape == (n, 10, 10, 640 if program == "robust" else 320)
    if program == "robust":
        assert op.split_w
        a, b = np.ascontiguousarray(src[..., :320]).view(np.uint16), np.ascontiguousarray(src[..., 320:]).view(np.uint16)
        assert (a == b).all(), "[x | x]: the two copies of Conv_1's source differ in %d of %d elements" % (int((a != b).sum()), a.size)
    res = R.reference(op, synth_weights, src, None, 16)          # robust: K = [hi | lo] over [x | x] = W_hi x + W_lo x
    rep = R.Report()
    worst, acc = R._compare(rep, op, idx, "", dst, res.ref, res.T, res.r, False, True, list(range(n)))
    print("\nConv_1, %s program, batch %d: worst err / tol %.3f, share of the accumulation allowance %.3f, %d elements"
          % (program, n, worst, acc, rep.elements))
    assert np.abs(res.ref).max() > 0.0, "the reference is all zeros: nothing would be checked"
    assert not rep.failures, "\n".join(rep.failures)
    assert worst <= 1.0


@pytest.mark.parametrize("batch", [8, 7])
def test_robust_program_read_one_copy_for_both_weight_halves(runs, synth_weights, batch):
    src, dst = runs("robust", batch)
    _check("robust", synth_weights, src, dst)


@pytest.mark.parametrize("batch", sorted({FIRST_BATCH, FIRST_BATCH - 1} - {0}))
def test_robust_program_at_the_routing_threshold(runs, synth_weights, batch):
    """The first batch on the GEMM kernel and the last one below it (the older kernel: the same bound holds there)."""
    src, dst = runs("robust", batch)
    _check("robust", synth_weights, src, dst)


def test_default_program_plain_form(runs, synth_weights):
    src, dst = runs("default", 8)
    _check("default", synth_weights, src, dst)


def test_a_frame_does_not_depend_on_its_batch(runs):
    """Batch 8, the same frames reversed, and the first seven of them: every frame's source AND Conv_1 tensor are the same bytes."""
    s8, d8 = runs("robust", 8)
    sr, dr = runs("robust", 8, True)
    s7, d7 = runs("robust", 7)
    bits = lambda t: np.ascontiguousarray(t).view(np.uint16)      # noqa: E731
    for f in range(8):
        assert (bits(s8[f]) == bits(sr[7 - f])).all(), "frame %d: Conv_1's source differs between a batch and its reverse" % f
        assert (bits(d8[f]) == bits(dr[7 - f])).all(), "frame %d: Conv_1 differs between a batch and its reverse" % f
    for f in range(7):
        assert (bits(s8[f]) == bits(s7[f])).all(), "frame %d: Conv_1's source differs between batch 8 and batch 7" % f
        assert (bits(d8[f]) == bits(d7[f])).all(), "frame %d: Conv_1 differs between batch 8 and batch 7" % f
    assert len({bits(d8[f]).tobytes() for f in range(8)}) == 8     # (eight different frames: the comparison is not vacuous)


def test_graph_nodes_do_not_depend_on_the_batch(model_dir_robust):
    """The kernel replaces Conv_1's launch one for one: the captured graph of the robust program has as many nodes at batch 8 (the GEMM
    kernel) as at batch 1 (tests/test_gpu_hp2.py pins the number; here only the equality)."""
    script = (
        "import sys, json, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from watsor_amd.runtime import HipEngine, ROW_DTYPE\n"
        "from watsor_amd.synth import synthetic_frame\n"
        "e = HipEngine(%r, 0, 8, 640, 480)\n"
        "out = {}\n"
        "for n in (8, 1):\n"
        "    frames = [synthetic_frame(640, 480, 6200 + i) for i in range(n)]\n"
        "    rows = [np.zeros(100, ROW_DTYPE) for _ in frames]\n"
        "    e.detect_batch(frames, rows)\n"
        "    out[str(n)] = e.graph_nodes(0)\n"
        "print(json.dumps(out))\n"
        "e.close()\n" % (conftest.ROOT, os.path.join(model_dir_robust, "mi355x.bin")))
    p = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, WZ_GRAPH="1"), capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-1500:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["8"] > 0 and out["8"] == out["1"], out

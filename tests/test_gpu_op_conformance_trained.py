"""Op-by-op conformance on the MI355X on weights spread like a trained checkpoint's (tests/trained_like.py): the walker, the bound and
the asserts of test_gpu_op_conformance.py, on per-channel amplitudes spread over up to two decades, with dead channels (gamma exactly
0: a zero weight column in both halves, the output the constant relu6(beta)) and saturating ones (6, code 65535, z = 1 at nearly every
pixel).  What the seeded one-scale weights never show a kernel: fp16-subnormal weights (the lo half of a split weight whose hi is about
1e-3), fp16-subnormal activations and results, the low end of the chunk buffer's codes under depthwise taps up to 100 x larger, and
the two MobileNet-v1 programs and Inception-v2 on anything but He-initialised weights.

  program                                   decades   batches
  MobileNet-v2 robust `-p 16`               2.0       1, 3      what `--robust auto` packs for such weights, and what bench.py times
  MobileNet-v2 robust `-p 16`               1.0       2
  MobileNet-v2 default `-p 16`              0.4       1, 3      the most the builder hands the default program
  MobileNet-v2 default `-p 16`              2.0       1         (the end-to-end score bar does not hold there; the per-op bound must)
  MobileNet-v2 one op per layer `-p 16`     2.0       1, 3
  MobileNet-v2 `-p 32`                      2.0       1
  MobileNet-v1 fused, one op per layer      1.5       1, 3 each
  MobileNet-v1 `-p 32`                      1.5       1
  Inception-v2 `-p 16`                      1.5       1, 3
  Inception-v2 `-p 32`                      1.5       1

The launchers' decisions by batch size are test_gpu_op_conformance.py's subject and do not depend on the weights: batch 1 (a synthetic
frame) takes the small-batch rules, batch 3 (noise of amplitude 4, impulses, zeros) the first large-batch shape with frame seams inside
a workgroup, all frames checked.

No test passes on nothing: each counts the compared elements whose reference is a non-zero fp16 subnormal, those in dead and those in
saturated channels, and requires all three to be above zero.  A dead channel of a `-p 16` tensor is compared bit for bit with
fp16(relu6(beta)) (op_reference.walk, `marks`): nothing but the bias reaches that store, so a wrong constant is a layout bug."""
import os
import time

import pytest

import conftest
import op_reference as R
import parity_utils as pu
import trained_like as TL
from watsor_amd import arch, engine, inception, mobilenet_v1
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

pytestmark = pytest.mark.gpu

SEED = 1234
TL_SEED = 77

# family -> (seeded weights, the one-op-per-layer program the generator walks)
FAMILIES = {
    "mobilenet_v2": (synthetic_weights, lambda: arch.build(fuse=False)),
    "mobilenet_v1": (synthetic_mobilenet_v1, lambda: mobilenet_v1.build(fuse=False)),
    "inception_v2": (synthetic_inception_v2, lambda: inception.build()),
}
_ROBUST = (dict(robust=True), lambda: arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True), 17, R.FLOAT_FORM_UPTO)
_DEFAULT = (dict(), lambda: arch.build(hp_upto=arch.HP_LAST_BLOCK), 17, -1)
# program -> (family, decades, precision, engine.build_engine arguments, the arch.Program that call packs, fused blocks in it, the last
#             block with the float-form chunk buffer, batches)
PROGRAMS = {
    "mobilenet_v2_robust_p16_2.0":  ("mobilenet_v2", 2.0, 16) + _ROBUST + ((1, 3),),
    "mobilenet_v2_robust_p16_1.0":  ("mobilenet_v2", 1.0, 16) + _ROBUST + ((2,),),
    "mobilenet_v2_default_p16_0.4": ("mobilenet_v2", 0.4, 16) + _DEFAULT + ((1, 3),),
    "mobilenet_v2_default_p16_2.0": ("mobilenet_v2", 2.0, 16) + _DEFAULT + ((1,),),
    "mobilenet_v2_unfused_p16_2.0": ("mobilenet_v2", 2.0, 16, dict(fuse=False), lambda: arch.build(fuse=False), 0, -1, (1, 3)),
    "mobilenet_v2_p32_2.0":         ("mobilenet_v2", 2.0, 32, dict(), lambda: arch.build(fuse=False, input_pair=True), 0, -1, (1,)),
    "mobilenet_v1_fused_p16_1.5":   ("mobilenet_v1", 1.5, 16, dict(), lambda: mobilenet_v1.build(fuse=True), 0, -1, (1, 3)),
    "mobilenet_v1_unfused_p16_1.5": ("mobilenet_v1", 1.5, 16, dict(fuse=False), lambda: mobilenet_v1.build(fuse=False), 0, -1, (1, 3)),
    "mobilenet_v1_p32_1.5":         ("mobilenet_v1", 1.5, 32, dict(), lambda: mobilenet_v1.build(fuse=False, input_pair=True), 0, -1, (1,)),
    "inception_v2_p16_1.5":         ("inception_v2", 1.5, 16, dict(), lambda: inception.build(), 0, -1, (1, 3)),
    "inception_v2_p32_1.5":         ("inception_v2", 1.5, 32, dict(), lambda: inception.build(input_pair=True), 0, -1, (1,)),
}
START = {1: 0, 2: 1, 3: 1}     # batch -> the input kind of frame 0 (op_reference.conformance_batch): together all four kinds
CASES = [(name, n) for name, p in PROGRAMS.items() for n in p[7]]

_cache = {}


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """name -> (model directory, weights, program, marks), built on first use; the weights once per (family, decades)."""
    def get(name):
        if name not in _cache:
            family, decades, precision, kw, make_prog = PROGRAMS[name][:5]
            if (family, decades) not in _cache:
                make_weights, make_unfused = FAMILIES[family]
                _cache[(family, decades)] = TL.trained_like(make_weights(SEED), make_unfused(), decades, TL_SEED)
            weights = _cache[(family, decades)]
            d = tmp_path_factory.mktemp(name.replace(".", "_"))
            engine.save_engine(engine.build_engine(weights, precision, **kw), os.path.join(str(d), "mi355x.bin"))
            prog = make_prog()
            _cache[name] = (str(d), weights, prog, TL.marks(prog, weights, precision))
        return _cache[name]
    yield get
    _cache.clear()


def _frame_input(seed):
    return pu.oracle_input_half([synthetic_frame(640, 480, 9500 + seed)])[0]


def _keep_engine(path, max_batch):
    os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        return conftest.make_engine(path, max_batch=max_batch, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE")


@pytest.mark.parametrize("name,n", CASES, ids=["%s-b%d" % c for c in CASES])
def test_every_op_within_its_own_bound_on_trained_like_weights(packed, name, n):
    t0 = time.time()
    path, weights, prog, marks = packed(name)
    precision, n_blocks, float_form_upto = PROGRAMS[name][2], PROGRAMS[name][5], PROGRAMS[name][6]
    assert sum(op.kind == arch.OP_MBCONV for op in prog.ops) == n_blocks
    e = _keep_engine(path, n)
    try:
        assert {t[0] for t in e.tensors()} == {"input"} | {t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t}
        assert len(e.ops()) == len(prog.ops) and e.precision == precision
        x = R.conformance_batch(n, prog.size, START[n], n * 10 + START[n], _frame_input)
        rep = R.walk(e, prog, weights, x, precision, check=False, float_form_upto=float_form_upto, marks=marks)
        print("\n%s batch %d: %s\n  %s; %.1f s" % (name, n, rep.summary(), rep.populations(), time.time() - t0))
        assert not rep.failures, "%s batch %d: %d failure(s):\n  %s" % (name, n, len(rep.failures), "\n  ".join(rep.failures[:20]))
        assert rep.ops_mbconv == 0 and rep.blocks_checked == n_blocks and rep.ops_unchecked == 0 and rep.ops_checked == len(prog.ops)
        assert rep.elements > 0 and max(v[0] for v in rep.worst.values()) <= 1.0
        assert rep.subnormal_refs > 0 and rep.dead_elements > 0 and rep.saturated_elements > 0, rep.populations()
    finally:
        e.close()

"""Op-by-op conformance on the MI355X: every op of every program against the float64 reference of THAT op on the source tensor the GPU
itself produced (tests/op_reference.py: `walk`).  Upstream error cancels; what is compared is one kernel's fp32 summation order and its
one final rounding, against a bound derived from the number formats (never from a kernel): |got - ref| <= tol element by element, and
value for value where the order is a contract (max pool, the `-p 16` depthwise stages).

Programs: MobileNet-v2 one op per layer at `-p 16` and `-p 32`, and of the default and the robust `-p 16` programs every op that is not
a fused block (Conv_1 -- with split weights in the robust one --, the extras pairs, the six heads on the wide kernel); Inception-v2 at
`-p 16` and `-p 32` (the 38 branch intermediates included); MobileNet-v1 unfused and fused (OP_DWSEP) at `-p 16`, and `-p 32`.
Batches 1, 2, 3, 8, 16, 21 for `-p 16` (the launchers choose split-K counts, tiles, column groups and the wide head kernel by the
batch's pixel count), 1 and 3 for `-p 32`; at 16 and 21 the references are computed for frame 0, a middle one and the last.
Inputs, a different one in every frame: preprocessed synthetic frames, fp16 noise of amplitude 4, impulses in corners / edges / centre,
all zeros (op_reference.conformance_batch).

The walker asserts its own coverage: every op checked or a fused block (OP_MBCONV: own tests, intermediates never leave LDS), every
channel of every other tensor written by exactly one checked op, every row of the 1917 x 4 / 1917 x 91 outputs by exactly one head."""
import os

import pytest

import conftest
import op_reference as R
import parity_utils as pu
from watsor_amd import arch, engine, inception, mobilenet_v1
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

pytestmark = pytest.mark.gpu

SEED = 1234

# program -> (weights, precision, engine.build_engine arguments, the arch.Program that builder call packs, fused blocks in it)
PROGRAMS = {
    "mobilenet_v2_unfused_p16": (synthetic_weights, 16, dict(fuse=False), lambda: arch.build(fuse=False), 0),
    "mobilenet_v2_p32":         (synthetic_weights, 32, dict(), lambda: arch.build(fuse=False, input_pair=True), 0),
    "mobilenet_v2_default_p16": (synthetic_weights, 16, dict(), lambda: arch.build(hp_upto=arch.HP_LAST_BLOCK), 17),
    "mobilenet_v2_robust_p16":  (synthetic_weights, 16, dict(robust=True),
                                 lambda: arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True), 17),
    "inception_v2_p16":         (synthetic_inception_v2, 16, dict(), lambda: inception.build(), 0),
    "inception_v2_p32":         (synthetic_inception_v2, 32, dict(), lambda: inception.build(input_pair=True), 0),
    "mobilenet_v1_unfused_p16": (synthetic_mobilenet_v1, 16, dict(fuse=False), lambda: mobilenet_v1.build(fuse=False), 0),
    "mobilenet_v1_fused_p16":   (synthetic_mobilenet_v1, 16, dict(), lambda: mobilenet_v1.build(fuse=True), 0),
    "mobilenet_v1_p32":         (synthetic_mobilenet_v1, 32, dict(), lambda: mobilenet_v1.build(fuse=False, input_pair=True), 0),
}
# batch -> the input kind of frame 0 of each pass (op_reference.conformance_batch): the small batches together see all four kinds
PASSES_P16 = {1: (0, 1), 2: (2,), 3: (0,), 8: (0,), 16: (1,), 21: (2,)}
PASSES_P32 = {1: (0,), 3: (1,)}
CASES = [(name, n) for name, spec in PROGRAMS.items() for n in (PASSES_P32 if spec[1] == 32 else PASSES_P16)]

_cache = {}


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """name -> (model directory, weights, program), built on first use."""
    def get(name):
        if name not in _cache:
            make_weights, precision, kw, make_prog, _ = PROGRAMS[name]
            if make_weights not in _cache:
                _cache[make_weights] = make_weights(SEED)
            d = tmp_path_factory.mktemp(name)
            engine.save_engine(engine.build_engine(_cache[make_weights], precision, **kw), os.path.join(str(d), "mi355x.bin"))
            _cache[name] = (str(d), _cache[make_weights], make_prog())
        return _cache[name]
    yield get
    _cache.clear()


def _frame_input(seed):
    return pu.oracle_input_half([synthetic_frame(640, 480, 9000 + seed)])[0]


def _keep_engine(path, max_batch):
    os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        return conftest.make_engine(path, max_batch=max_batch, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE")


@pytest.mark.parametrize("name,n", CASES, ids=["%s-b%d" % c for c in CASES])
def test_every_op_within_its_own_bound(packed, name, n):
    path, weights, prog = packed(name)
    precision, n_blocks = PROGRAMS[name][1], PROGRAMS[name][4]
    e = _keep_engine(path, n)
    try:
        # the program is the one the engine holds: same tensors, same ops
        assert {t[0] for t in e.tensors()} == {"input"} | {t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t}
        assert len(e.ops()) == len(prog.ops) and e.precision == precision
        for start in (PASSES_P32 if precision == 32 else PASSES_P16)[n]:
            x = R.conformance_batch(n, prog.size, start, n * 10 + start, _frame_input)
            rep = R.walk(e, prog, weights, x, precision, frames=R.frame_subset(n), check=False)
            print("\n%s batch %d (first input kind %d): %s" % (name, n, start, rep.summary()))
            assert not rep.failures, "%s batch %d: %d failure(s):\n  %s" % (name, n, len(rep.failures), "\n  ".join(rep.failures[:20]))
            assert rep.ops_mbconv == n_blocks and rep.ops_unchecked == 0 and rep.ops_checked == len(prog.ops) - n_blocks
            assert rep.elements > 0 and max(v[0] for v in rep.worst.values()) <= 1.0
    finally:
        e.close()

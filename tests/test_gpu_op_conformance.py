"""Op-by-op conformance on the MI355X: every op of every program against the float64 reference of THAT op on the source tensor the GPU
itself produced (tests/op_reference.py: `walk`).  Upstream error cancels; what is compared is one kernel's fp32 summation order and its
roundings, against a bound derived from the number formats (never from a kernel): |got - ref| <= tol element by element, and
value for value where the order is a contract (max pool, the `-p 16` depthwise stages).

Programs: MobileNet-v2 one op per layer at `-p 16` and `-p 32`; the four FUSED `-p 16` programs -- default, robust, `--plain-fp16` and
the one with the stem as its own kernel -- whose 17 inverted-residual blocks (OP_MBCONV) are checked like any other op
(op_reference.block_reference: three stages, the chunk buffer's format, the pair stores; block 13's expanded tensor as a second
output; the exact properties of every stored pair); Inception-v2 at `-p 16` and `-p 32` (the 38 branch intermediates included);
MobileNet-v1 unfused and fused (OP_DWSEP) at `-p 16`, and `-p 32`.

Batches 1, 2, 3, 8, 16, 21 for the unfused `-p 16` programs (the launchers choose split-K counts, tiles, column groups and the wide head
kernel by the batch's pixel count), 1 and 3 for `-p 32`.  The default and the robust program add the sizes at which the block
launchers' decision lists (k_mbconv_hp.hip: wz_hp_pick_q, wz_hp_pick; k_mbconv_hp2.hip) change shape:
   1   the small-batch rules (blocks 1 - 3 chunk-split, 4 x 4 tiles on blocks 2, 4, 5: n <= 2); `few` (at most 64 workgroups of the
       one-wave-per-tile launch) holds on every map, the 75x75 one included (19 x 10 tiles / 4 = 48 workgroups)
   2   the small-batch rules with two frames: a one-wave-per-tile workgroup of four tiles holds tiles of both; `few` is off on 75x75
   3   the first large-batch shape (one wave per tile, 4 x 8 tiles), frame seams inside a workgroup
   5   `few` still holds on the 38x38 maps (10 x 5 tiles x 5 / 4 = 63 workgroups); 500 pixels of launch B are 31.25 tiles of 16: the
       last one is part garbage.  Launch A runs two waves per chunk while one wave per chunk would give at most 128 workgroups on an idle
       chip (block 13, 25 n: n <= 5; blocks 14 .. 16, 16 n: n <= 8) and at most 64 otherwise, which is what the stage entry points of
       this test ask for: block 13 changes between 2 and 3, blocks 14 .. 16 between 3 and 5
   6   `few` is off on the 38x38 maps (75 workgroups)
   8   the idle-chip rule's last batch for blocks 14 .. 16; 800 pixels = 50 whole tiles
   9   ... its first batch on the other side; 900 pixels = 56.25 tiles
  16   what the unfused programs run as well
  21   an odd batch beyond every threshold: 2100 pixels = 131.25 tiles, 21 x 25 = 525 tiles of the 19x19 maps
The `--plain-fp16` and stem-separate programs run their blocks on kernels whose launchers choose nothing by the batch size
(k_mbconv.hip, k_mbconv_cs.hip, k_mbconv_wave.hip): 1, 2 (two frames' tiles in one workgroup of the wave kernel), 3 and 21.
Frames: all of them up to batch 3 for the fused programs (8 for the others); beyond, frame 0, a middle one and the last.
Inputs, a different one in every frame: preprocessed synthetic frames, fp16 noise of amplitude 4 (drives both clamps of the chunk
buffer), impulses in corners / edges / centre and all zeros (the out-of-frame halo) (op_reference.conformance_batch).

The walker asserts its own coverage: every op checked, every channel of every tensor other than the input written by exactly one
checked op, every row of the 1917 x 4 / 1917 x 91 outputs by exactly one head."""
import os

import pytest

import conftest
import op_reference as R
import parity_utils as pu
from watsor_amd import arch, engine, inception, mobilenet_v1
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

pytestmark = pytest.mark.gpu

SEED = 1234

# program -> (weights, precision, engine.build_engine arguments, the arch.Program that builder call packs, fused blocks in it,
#             the last block with the float-form chunk buffer)
PROGRAMS = {
    "mobilenet_v2_unfused_p16": (synthetic_weights, 16, dict(fuse=False), lambda: arch.build(fuse=False), 0, -1),
    "mobilenet_v2_p32":         (synthetic_weights, 32, dict(), lambda: arch.build(fuse=False, input_pair=True), 0, -1),
    "mobilenet_v2_default_p16": (synthetic_weights, 16, dict(), lambda: arch.build(hp_upto=arch.HP_LAST_BLOCK), 17, -1),
    "mobilenet_v2_robust_p16":  (synthetic_weights, 16, dict(robust=True),
                                 lambda: arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True), 17, R.FLOAT_FORM_UPTO),
    "mobilenet_v2_plain_p16":   (synthetic_weights, 16, dict(hp_upto=-1), lambda: arch.build(hp_upto=-1), 17, -1),
    "mobilenet_v2_stem_separate_p16": (synthetic_weights, 16, dict(fuse_stem=False), lambda: arch.build(fuse_stem=False), 17, -1),
    "inception_v2_p16":         (synthetic_inception_v2, 16, dict(), lambda: inception.build(), 0, -1),
    "inception_v2_p32":         (synthetic_inception_v2, 32, dict(), lambda: inception.build(input_pair=True), 0, -1),
    "mobilenet_v1_unfused_p16": (synthetic_mobilenet_v1, 16, dict(fuse=False), lambda: mobilenet_v1.build(fuse=False), 0, -1),
    "mobilenet_v1_fused_p16":   (synthetic_mobilenet_v1, 16, dict(), lambda: mobilenet_v1.build(fuse=True), 0, -1),
    "mobilenet_v1_p32":         (synthetic_mobilenet_v1, 32, dict(), lambda: mobilenet_v1.build(fuse=False, input_pair=True), 0, -1),
}
# batch -> the input kind of frame 0 of each pass (op_reference.conformance_batch): the small batches together see all four kinds
PASSES_P16 = {1: (0, 1), 2: (2,), 3: (0,), 8: (0,), 16: (1,), 21: (2,)}
PASSES_P32 = {1: (0,), 3: (1,)}
PASSES_SPLIT = {1: (0, 1), 2: (2,), 3: (0,), 5: (1,), 6: (3,), 8: (0,), 9: (1,), 16: (1,), 21: (2,)}   # the split-operand launchers' thresholds (above)
PASSES_PLAIN = {1: (0, 1), 2: (2,), 3: (0,), 21: (2,)}


def _passes(name):
    _, precision, kw, _, n_blocks, _ = PROGRAMS[name]
    if precision == 32:
        return PASSES_P32
    if not n_blocks:
        return PASSES_P16
    return PASSES_PLAIN if (kw.get("hp_upto") == -1 or kw.get("fuse_stem") is False) else PASSES_SPLIT


CASES = [(name, n) for name in PROGRAMS for n in _passes(name)]

_cache = {}


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    """name -> (model directory, weights, program), built on first use."""
    def get(name):
        if name not in _cache:
            make_weights, precision, kw, make_prog = PROGRAMS[name][:4]
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
    precision, n_blocks, float_form_upto = PROGRAMS[name][1], PROGRAMS[name][4], PROGRAMS[name][5]
    assert sum(op.kind == arch.OP_MBCONV for op in prog.ops) == n_blocks
    e = _keep_engine(path, n)
    try:
        # the program is the one the engine holds: same tensors, same ops
        assert {t[0] for t in e.tensors()} == {"input"} | {t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t}
        assert len(e.ops()) == len(prog.ops) and e.precision == precision
        for start in _passes(name)[n]:
            x = R.conformance_batch(n, prog.size, start, n * 10 + start, _frame_input)
            rep = R.walk(e, prog, weights, x, precision, frames=R.frame_subset(n, 3 if n_blocks else 8), check=False,
                         float_form_upto=float_form_upto)
            print("\n%s batch %d (first input kind %d): %s" % (name, n, start, rep.summary()))
            assert not rep.failures, "%s batch %d: %d failure(s):\n  %s" % (name, n, len(rep.failures), "\n  ".join(rep.failures[:20]))
            assert rep.ops_mbconv == 0 and rep.blocks_checked == n_blocks and rep.ops_unchecked == 0 and rep.ops_checked == len(prog.ops)
            assert rep.elements > 0 and max(v[0] for v in rep.worst.values()) <= 1.0
    finally:
        e.close()

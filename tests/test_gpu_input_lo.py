"""The lo half of a pair input is consumed by the first op, shown with the lo half as the whole signal.

In a real batch lo is 2^-12 of the input: a first op that dropped it, or took it from a neighbouring pixel or channel, could hide
inside the op's own bound (tests/test_gpu_production_walk.py checks it there, to within that bound).  Block 0 of the default and of
the robust program -- the stem gather of k_mbconv_hp.hip -- computes Whi.xhi + Whi.xlo + Wlo.xhi for ANY two halves, and
op_reference.block_reference models exactly that (its T1 carries |xlo|).  So the block runs on uploaded inputs (stage_block_at) whose
lo half is as large as the hi half:
    hi = 0, lo = x        everything the block stores comes from the lo half
    hi = x, lo = y        both of order one: lo from the wrong place would be an error of order one
x, y: a preprocessed frame, fp16 noise of amplitude 4, impulses (the makers of op_reference.conformance_batch), one frame and two
(a frame seam inside a workgroup).  The stored output is compared with block_reference on exactly those halves, under its own
tolerance, and with the exact properties of a stored pair.

The comparison has power by a check on the reference side alone: against the tolerance of block_reference(hi, 0) -- a block that
ignored lo -- the GPU's output must lie OUTSIDE in at least 1 % of the elements of every frame (printed).  No kernel is modified."""
import numpy as np
import pytest

import hp_halo_gather as hg
import op_reference as R
import parity_utils as pu
from watsor_amd import arch
from watsor_amd.synth import synthetic_frame

pytestmark = pytest.mark.gpu

POWER = 0.01
FLOAT_FORM_UPTO = {"default": -1, "robust": R.FLOAT_FORM_UPTO}


def _frame(seed):
    return pu.oracle_input_half([synthetic_frame(640, 480, 9300 + seed)])[0]


def _noise(seed):
    return R.noise_input(arch.INPUT_SIZE, 500 + seed)


def _impulses(seed):
    return R.impulse_input(arch.INPUT_SIZE, 700 + seed)


def _zeros(seed):
    return np.zeros((arch.INPUT_SIZE, arch.INPUT_SIZE, 4), np.float16)


# case -> per frame (maker of hi, maker of lo).  Every lo is dense (a frame or noise), so that the power check has something to see
# in every frame; the impulses -- corners, edges, centre -- sit in hi, next to a dense lo.
CASES = {
    "1-lo_only_noise":      [(_zeros, _noise)],
    "1-lo_only_frame":      [(_zeros, _frame)],
    "1-impulses_and_noise": [(_impulses, _noise)],
    "1-frame_and_noise":    [(_frame, _noise)],
    "2-lo_only":            [(_zeros, _frame), (_zeros, _noise)],
    "2-both":               [(_frame, _noise), (_noise, _frame)],
}


@pytest.fixture(scope="module")
def engines(tmp_path_factory, synth_weights):
    """program -> (engine with every tensor in a buffer of its own, arch.Program), created on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (hg.make_engine(name, str(tmp_path_factory.mktemp("input_lo_" + name)), synth_weights), hg.program(name))
        return made[name]
    yield get
    for e, _ in made.values():
        e.close()


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", list(hg.PROGRAMS))
def test_block_0_on_a_lo_half_of_order_one(engines, synth_weights, name, case):
    e, prog = engines(name)
    idx, op = next((i, op) for i, op in enumerate(prog.ops) if op.kind == arch.OP_MBCONV and op.block == 0)
    assert op.stem and op.hp and op.src == "input" and prog.tensors["input"].hp and prog.tensors[op.dst].hp and not op.res
    makers = CASES[case]
    n, S = len(makers), prog.size
    hi = np.stack([mh(10 * f) for f, (mh, _) in enumerate(makers)])
    lo = np.stack([ml(10 * f + 1) for f, (_, ml) in enumerate(makers)])
    assert hi.shape == lo.shape == (n, S, S, 4) and hi.dtype == lo.dtype == np.float16
    assert not hi[..., 3].any() and not lo[..., 3].any() and all((lo[f, ..., :3] != 0).mean() > 0.9 for f in range(n))
    names = [t[0] for t in e.tensors()]
    dst = names.index(op.dst)
    e.stage_forward(np.zeros((n, S, S, 4), np.float16))                  # the batch whose block 0 runs again, on an all-zero input
    before = hg.read_raw(e, dst, n).copy()
    d = e.upload(np.concatenate([hi, lo], axis=-1))                      # a pair tensor as stored: per pixel four hi halves, four lo halves
    try:
        e.stage_block_at(idx, n, d)
    finally:
        e.free(d)
    assert (hg.read_raw(e, dst, n) != before).any()                      # the entry point ran the block
    got = [e.stage_read_tensor(dst, f, halves=True) for f in range(n)]
    gh, gl = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    form = R.chunk_form(op, FLOAT_FORM_UPTO[name])
    res = R.block_reference(op, synth_weights, hi, lo, None, None, form, "pair")
    rep = R.Report()
    worst, acc = R._compare(rep, op, idx, "", gh.astype(np.float64) + gl.astype(np.float64), res.ref, None, None, False, True, list(range(n)),
                            tol=res.tol, acc=res.acc, kind=R.op_kind_name(op, FLOAT_FORM_UPTO[name]))
    rep.failures += R.pair_checks(gh, gl)
    # the same output against a block that ignores the lo half: outside its tolerance in at least POWER of every frame's elements
    blind = R.block_reference(op, synth_weights, hi, np.zeros_like(lo), None, None, form, "pair")
    outside = (np.abs(gh.astype(np.float64) + gl.astype(np.float64) - blind.ref) > blind.tol).reshape(n, -1).mean(axis=1)
    print("\n%s, %s: worst err / tol %.3g (acc %.3g), %d elements; outside the tolerance of the reference without lo, per frame: %s"
          % (name, case, worst, acc, rep.elements, " ".join("%.4f" % v for v in outside)))
    assert not rep.failures, "\n  ".join(rep.failures)
    assert worst <= 1.0
    assert outside.min() >= POWER, outside

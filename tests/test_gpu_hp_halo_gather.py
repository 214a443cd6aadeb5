"""The halo loads of the split-operand blocks (k_mbconv_hp.hip, launch A of k_mbconv_hp2.hip) return the bytes they returned on the
commit that recorded tests/golden/hp_halo_gather.json, or zeros where a lane has nothing to read: the blocks' output tensors are
equal bit for bit (tests/hp_halo_gather.py says which blocks, batches and inputs, and why those).

  * the network on op_reference.conformance_batch at batches 1, 2, 3 and 5 (the sizes at which the launchers' decision lists change
    shape), robust and default program: SHA-256 of each listed block's output tensor(s) of every frame;
  * each listed block again on its own with its two-frame input inside a larger allocation whose other bytes are fp16 NaN patterns
    (wz_stage_block_at): the same hashes and no NaN in the output -- a load outside the tensor would bring a NaN in, a border tap taken
    from the neighbouring frame other values.  A first run on an all-zero input in the same place shows that the entry point runs the
    block (its output changes) before the real input brings the recorded tensor back -- once as the network launches the block, once
    with one frame per launch (what a batch of 2^31 bytes of block input and more gets: every launch's descriptor then covers its own
    frame only)."""
import numpy as np
import pytest

import hp_halo_gather as hg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return hg.load_golden()


@pytest.fixture(scope="module")
def engines(tmp_path_factory, synth_weights):
    """program -> (engine, arch.Program), created on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (hg.make_engine(name, str(tmp_path_factory.mktemp("hp_halo_" + name)), synth_weights), hg.program(name))
        return made[name]
    yield get
    for e, _ in made.values():
        e.close()


@pytest.mark.parametrize("n", hg.BATCHES)
@pytest.mark.parametrize("name", list(hg.PROGRAMS))
def test_block_outputs_bit_for_bit(engines, golden, name, n):
    e, prog = engines(name)
    got = hg.hashes_of_batch(e, prog, n)
    assert sorted(got) == sorted(str(b) for b in hg.BLOCKS)
    assert got == golden[name][str(n)]


@pytest.mark.parametrize("block", hg.BLOCKS)
@pytest.mark.parametrize("name", list(hg.PROGRAMS))
def test_input_inside_nan_guard(engines, golden, name, block):
    e, prog = engines(name)
    n = hg.GUARD_BATCH
    want = golden[name][str(n)][str(block)]
    e.stage_forward(hg.batch_input(n, prog.size))
    idx, op = hg.block_ops(prog)[block]
    assert hg.block_hash(e, op, n) == want
    src = hg.read_raw(e, [t[0] for t in e.tensors()].index(op.src), n).reshape(-1)
    guard = np.resize(np.array(hg.NAN_PATTERNS, np.uint16), hg.GUARD_BYTES // 2)
    assert np.isnan(guard.view(np.float16)).all()
    for fill, launch_frames, same in ((np.zeros_like(src), 0, False), (src, 0, True), (np.zeros_like(src), 1, False), (src, 1, True)):
        d = e.upload(np.concatenate([guard, fill, guard]))
        try:
            e.stage_block_at(idx, n, d + hg.GUARD_BYTES, launch_frames)
            assert (hg.block_hash(e, op, n) == want) == same
            for t in hg.block_tensors(e, op):
                assert not np.isnan(hg.read_raw(e, t, n).view(np.float16)).any()
        finally:
            e.free(d)

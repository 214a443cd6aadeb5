"""The output tensors of the split-operand blocks, pinned bit for bit: what tests/golden/hp_halo_gather.json records
(tests/golden/make_hp_halo_gather_golden.py writes it, on the commit whose tensors are to be kept) and
tests/test_gpu_hp_halo_gather.py compares.

The halo loads of k_mbconv_hp.hip and of launch A of k_mbconv_hp2.hip decide which bytes a block reads: a load that returns other
bytes than before -- a tap of the neighbouring frame, a pixel beyond the tile's halo, a channel chunk beyond cin0 -- changes the
block's output, and nothing else in these hashes can.  Blocks 0 (the stem gather), 1, 3, 6 (stride 2), 2, 4 (stride 1, large maps),
7 (38x38 ... 19x19), 11 (19x19, lean builds) and 13 (robust program: launch A of the two-launch form; its expanded tensor, the first
SSD feature map, is stored by launch A itself, its output tensor by launch B from launch A's fragments)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "hp_halo_gather.json")

SEED = 1234
PROGRAMS = {"robust": dict(robust=True), "default": {}}
BLOCKS = (0, 1, 2, 3, 4, 6, 7, 11, 13)
# batch -> the input kind of frame 0 (op_reference.conformance_batch: frame, noise, impulses, zeros in turn): together every kind;
# the two-frame batch is frame + noise -- dense on both sides of the frame seam
START = {1: 2, 2: 0, 3: 1, 5: 0}
BATCHES = tuple(START)
MAX_BATCH = 5
GUARD_BATCH = 2
GUARD_BYTES = 1 << 16          # on each side of the tensor: more than two rows of the widest input (300 x 16 bytes, 150 x 64 bytes)
NAN_PATTERNS = (0x7E00, 0x7FFF, 0xFE00, 0x7C01)


def program(name):
    from watsor_amd import arch
    return arch.build(hp_upto=arch.HP_ALL_BLOCKS, conv1_split=True) if name == "robust" else arch.build(hp_upto=arch.HP_LAST_BLOCK)


def make_engine(name, tmp_dir, weights):
    """The program's engine on the development library with every tensor in a buffer of its own."""
    from watsor_amd import engine
    from watsor_amd.runtime import HipEngine
    path = os.path.join(tmp_dir, "hp_halo_%s.bin" % name)
    engine.save_engine(engine.build_engine(weights, **PROGRAMS[name]), path)
    os.environ["WZ_NO_BUFFER_REUSE"] = "1"
    try:
        return HipEngine(path, 0, MAX_BATCH, 1920, 1080, dev=True)
    finally:
        os.environ.pop("WZ_NO_BUFFER_REUSE")


def batch_input(n, size):
    import op_reference as R
    import parity_utils as pu
    from watsor_amd.synth import synthetic_frame
    return R.conformance_batch(n, size, START[n], n * 10 + START[n], lambda seed: pu.oracle_input_half([synthetic_frame(640, 480, 9000 + seed)])[0])


def block_ops(prog):
    """block -> (index of its op, the op)"""
    from watsor_amd import arch
    return {op.block: (i, op) for i, op in enumerate(prog.ops) if op.kind == arch.OP_MBCONV and op.block in BLOCKS}


def frame_bytes(e, idx):
    _, h, w, c = e.tensors()[idx]
    return h * w * c * 2 * (2 if e.tensor_is_pair(idx) else 1)


def read_raw(e, idx, n):
    """Tensor `idx` of frames 0 .. n - 1 exactly as stored: uint16 [n][halves per frame]."""
    out = np.empty((n, frame_bytes(e, idx) // 2), np.uint16)
    for f in range(n):
        row = np.empty(out.shape[1], np.uint16)
        e._ck(e._lib.wz_stage_read_tensor(e._h, idx, f, C.c_void_p(row.ctypes.data)))
        out[f] = row
    return out


def block_tensors(e, op):
    names = [t[0] for t in e.tensors()]
    return [names.index(t) for t in (op.dst, op.dst2) if t]


def block_hash(e, op, n):
    h = hashlib.sha256()
    for idx in block_tensors(e, op):
        h.update(read_raw(e, idx, n).tobytes())
    return h.hexdigest()


def hashes_of_batch(e, prog, n):
    """Runs the network on the batch's input; block -> SHA-256 of its output tensor(s) of all n frames as stored."""
    e.stage_forward(batch_input(n, prog.size))
    return {str(b): block_hash(e, op, n) for b, (_, op) in sorted(block_ops(prog).items())}


def load_golden():
    with open(PATH) as f:
        return json.load(f)


def write_golden(cases):
    with open(PATH, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")

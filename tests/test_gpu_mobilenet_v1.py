"""SSD-MobileNet-v1 engines on the MI355X (watsor_amd/mobilenet_v1.py, csrc/k_dwsep.hip): every tensor against the CPU oracle of
tests/mobilenet_v1_oracle.py for the fused and the one-op-per-layer `-p 16` programs and for `-p 32`, the fused separable layers
bit for bit against the unfused ones, the plugin end to end, batches, the asynchronous / bound / graph-replayed paths, all three
networks in one process, and the load-time refusal of a separable layer the kernel does not cover.

Tolerances are those of tests/test_gpu_inception.py: `-p 32` agrees with the fp32 oracle to fp32 rounding (tensors 1e-4 of their
range, scores 1e-4); `-p 16` keeps the plain fp16 programs' LOGIT_TOL / BOXENC_TOL on the heads and 1e-3 on the scores (the CPU
emulation of this program: 4.5e-4, profiles/mobilenet_v1_fp16_emulation.json)."""
import os
import struct

import numpy as np
import pytest

import conftest
import parity_utils as pu
from inception_v2_oracle import InceptionOracleDetector
from mobilenet_v1_oracle import MobilenetV1OracleDetector, MobilenetV1OracleNet
from oracle import detect as odet
from oracle.compare import assert_rows_match
from oracle.postprocess import sigmoid
from watsor_amd import arch, engine
from watsor_amd.runtime import FMT_RGB24, ROW_DTYPE
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1

pytestmark = pytest.mark.gpu

LOGIT_TOL = 0.05
BOXENC_TOL = 0.04
SCORE_TOL = 1e-3
SEED = 1234


@pytest.fixture(scope="module")
def v1_weights():
    return synthetic_mobilenet_v1(SEED)


@pytest.fixture(scope="module")
def v1_dirs(tmp_path_factory, v1_weights):
    """fused / unfused `-p 16` and `-p 32` engine directories."""
    out = {}
    for key, p, fuse in (("p16", 16, True), ("p16_unfused", 16, False), ("p32", 32, False)):
        d = tmp_path_factory.mktemp("mobilenet_v1_" + key)
        engine.save_engine(engine.build_engine(v1_weights, p, fuse=fuse), os.path.join(str(d), "mi355x.bin"))
        out[key] = str(d)
    return out


@pytest.fixture(scope="module")
def frames():
    return [synthetic_frame(640, 480, 5100 + i) for i in range(2)]


@pytest.fixture(scope="module")
def oracle_out(v1_weights, frames):
    x_half = pu.oracle_input_half(frames)
    be, lg, T = pu.oracle_forward_from_half(MobilenetV1OracleNet(v1_weights), x_half, keep=True)
    return x_half, be, lg, T


def _keep_engine(path, max_batch=2, **env):
    env = dict(env, WZ_NO_BUFFER_REUSE="1")
    os.environ.update(env)
    try:
        return conftest.make_engine(path, max_batch=max_batch, dev=True)
    finally:
        for k in env:
            os.environ.pop(k)


@pytest.mark.parametrize("program", ["p16_unfused", "p16", "p32"])
def test_every_tensor_close_to_oracle(v1_dirs, oracle_out, program):
    x_half, rbe, rlg, T = oracle_out
    e = _keep_engine(v1_dirs[program])
    try:
        kinds = [o["kind"] for o in e.ops()]
        assert (arch.OP_DWSEP in kinds) == (program == "p16")
        be, lg = e.stage_forward(x_half)
        worst = {}
        for idx, (name, h, w, c) in enumerate(e.tensors()):
            if name == "input":
                continue
            got = np.stack([e.stage_read_tensor(idx, f) for f in range(2)]).astype(np.float32)
            ref = T[name]
            assert got.shape == ref.shape, name
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            bound = (1e-4 * scale + 1e-5) if program == "p32" else (0.04 * scale + 0.02)
            assert err <= bound, "%s (%s): max abs err %.3g (max|ref| %.3f)" % (name, program, err, scale)
            worst[name] = err / max(scale, 1e-12)
        held = ["Conv2d_0", "Conv2d_1_pointwise", "Conv2d_11_pointwise", "Conv2d_13_pointwise"]
        if program != "p16":
            held += ["Conv2d_1_depthwise", "Conv2d_13_depthwise"]
        for name in held:
            assert name in worst, name
        print("\n%s: worst relative tensor error %.2e (%s)" % (program, max(worst.values()), max(worst, key=worst.get)))
        tol_b, tol_l = (1e-3, 1e-3) if program == "p32" else (BOXENC_TOL, LOGIT_TOL)
        assert np.abs(be - rbe).max() <= tol_b and np.abs(lg - rlg).max() <= tol_l
        dscore = float(np.abs(sigmoid(lg) - sigmoid(rlg)).max())
        print("%s: max |dscore| over all 1917 x 91 entries: %.2e" % (program, dscore))
        assert dscore <= (1e-4 if program == "p32" else SCORE_TOL)
    finally:
        e.close()


@pytest.mark.parametrize("n", [2, 16])
def test_fused_layers_equal_unfused_layers(v1_dirs, oracle_out, n):
    """One launch per separable layer (k_dwsep.hip) rounds at the same points and, with the unfused 1x1 convs not split along K
    (WZ_SPLITK=0), accumulates in the same order as wz_k_dw + wz_k_conv: every tensor both programs hold and the heads are
    bit-identical.  Batch 16 takes layers 6 .. 11 onto the widest column slice per wave (wz_k_dwsep<1, 8>)."""
    x_half = oracle_out[0] if n == 2 else pu.oracle_input_half([synthetic_frame(640, 480, 5200 + i) for i in range(n)])
    e_unf = _keep_engine(v1_dirs["p16_unfused"], max_batch=n, WZ_SPLITK="0")
    e_fus = _keep_engine(v1_dirs["p16"], max_batch=n, WZ_SPLITK="0")
    try:
        a = e_unf.stage_forward(x_half)
        b = e_fus.stage_forward(x_half)
        unf = {t[0]: i for i, t in enumerate(e_unf.tensors())}
        fused = e_fus.tensors()
        assert len(fused) == len(unf) - 13 and sum(o["kind"] == arch.OP_DWSEP for o in e_fus.ops()) == 13
        bad = []
        for idx, (name, h, w, c) in enumerate(fused):
            if name == "input":
                continue
            for f in range(n):
                x = e_fus.stage_read_tensor(idx, f)
                y = e_unf.stage_read_tensor(unf[name], f)
                if x.tobytes() != y.tobytes():
                    d = np.abs(x.astype(np.float32) - y.astype(np.float32))
                    bad.append("%s[%d]: %d of %d differ, max %.4g" % (name, f, int((d > 0).sum()), d.size, d.max()))
        assert not bad, "\n".join(bad[:12])
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    finally:
        e_unf.close()
        e_fus.close()


@pytest.mark.parametrize("program", ["p16", "p32"])
def test_detect_end_to_end_matches_oracle_detector(v1_dirs, v1_weights, program):
    """Rows through the plugin class against the oracle detector on 640x480, 1280x720 and 1920x1080 frames: scores within 1e-3,
    boxes within a pixel."""
    from watsor_amd.detection.hip_gpu import HipObjectDetector
    from watsor_amd.share import DetectionArray
    oracle = MobilenetV1OracleDetector(v1_weights)
    frames = [synthetic_frame(640, 480, 6100), synthetic_frame(1280, 720, 6101), synthetic_frame(1920, 1080, 6102)]
    with HipObjectDetector(v1_dirs[program], 0) as det:
        for f in frames:
            rows = DetectionArray()
            assert det.detect(f.shape, f, rows) > 0
            got = np.frombuffer(rows, dtype=ROW_DTYPE)
            b, c, s, _, _ = oracle.raw(f)
            r = assert_rows_match(got, odet.rows_as_array(f.shape, b, c, s), f.shape, tol=SCORE_TOL,
                                  what="%s %dx%d" % (program, f.shape[1], f.shape[0]))
            assert len(r["pairs"]) >= 90


@pytest.fixture(scope="module")
def batch_frames():
    sizes = [(640, 480), (1280, 720), (1920, 1080), (640, 480)]
    return [synthetic_frame(w, h, 7000 + i) for i, (w, h) in enumerate(sizes * 4)]   # 16 frames, mixed sizes (those of test_gpu_inception.py)


def test_batches_match_oracle(v1_dirs, v1_weights, batch_frames):
    """detect_batch at batch 1 .. 8 (mixed frame sizes) against the oracle detector, frame by frame."""
    oracle = MobilenetV1OracleDetector(v1_weights)
    refs = {}
    e = conftest.make_engine(v1_dirs["p16"], max_batch=8)
    try:
        for n in range(1, 9):
            fr = batch_frames[:n]
            rows = [np.zeros(100, ROW_DTYPE) for _ in fr]
            e.detect_batch(fr, rows)
            for i, (f, got) in enumerate(zip(fr, rows)):
                if i not in refs:
                    b, c, s, _, _ = oracle.raw(f)
                    refs[i] = odet.rows_as_array(f.shape, b, c, s)
                assert_rows_match(got, refs[i], f.shape, tol=SCORE_TOL, what="batch %d frame %d" % (n, i))
    finally:
        e.close()


def test_host_bound_and_replayed_paths_equal_detect_batch(v1_dirs, batch_frames):
    """wz_submit_host + wz_collect and the bound-frame path give the rows of wz_detect_batch bit for bit, with all lanes busy
    (graph replay) as well as one batch at a time (kernel by kernel)."""
    e = conftest.make_engine(v1_dirs["p16"], max_batch=8)
    try:
        batches = [batch_frames[0:3], batch_frames[3:8], batch_frames[8:9], batch_frames[9:13]]
        refs = []
        for b in batches:
            ref = [np.zeros(100, ROW_DTYPE) for _ in b]
            e.detect_batch(b, ref)
            refs.append(ref)
        assert e.num_slots >= len(batches)
        for rep in range(2):                   # the second round replays the graphs captured in the first
            for lane, b in enumerate(batches):
                e.submit_host(lane, b)
            for lane, b in enumerate(batches):
                got = [np.zeros(100, ROW_DTYPE) for _ in b]
                e.collect(lane, got)
                for g, r in zip(got, refs[lane]):
                    assert g.tobytes() == r.tobytes(), (rep, lane)
        flat = [f for b in batches for f in b]
        rows = np.zeros((len(flat), 100), ROW_DTYPE)
        e.bind_frames([f.ctypes.data for f in flat], [f.shape[1] for f in flat], [f.shape[0] for f in flat], [FMT_RGB24] * len(flat),
                      [-1] * len(flat), [rows[i].ctypes.data for i in range(len(flat))])
        entries, k = [], 0
        for b in batches:
            entries.append(list(range(k, k + len(b))))
            k += len(b)
        for lane, ent in enumerate(entries):
            e.submit_bound(lane, ent)
        for lane, ent in enumerate(entries):
            e.collect_bound(lane)
            for j, i in enumerate(ent):
                assert rows[i].tobytes() == refs[lane][j].tobytes(), (lane, j)
        e.bind_frames([], [], [], [], [], [])
    finally:
        e.close()


def test_three_networks_in_one_process(model_dir_default, synth_weights, v1_dirs, v1_weights, tmp_path):
    """MobileNet-v1, MobileNet-v2 and Inception-v2 engines open at once: each gives its own network's rows."""
    inc_w = synthetic_inception_v2(SEED)
    engine.save_engine(engine.build_engine(inc_w, 16), str(tmp_path / "mi355x.bin"))
    f = synthetic_frame(640, 480, 8100)
    e_v1 = conftest.make_engine(v1_dirs["p16"], max_batch=2)
    e_v2 = conftest.make_engine(model_dir_default, max_batch=2)
    e_in = conftest.make_engine(str(tmp_path), max_batch=2)
    try:
        pairs = ((e_v1, MobilenetV1OracleDetector(v1_weights)), (e_v2, odet.OracleObjectDetector(weights=synth_weights)),
                 (e_in, InceptionOracleDetector(inc_w)))
        for _ in range(2):
            for e, oracle in pairs:
                got = np.zeros(100, ROW_DTYPE)
                e.detect_batch([f], [got])
                b, c, s, _, _ = oracle.raw(f)
                assert_rows_match(got, odet.rows_as_array(f.shape, b, c, s), f.shape, tol=SCORE_TOL)
    finally:
        e_in.close()
        e_v2.close()
        e_v1.close()


def _patched_image(src_dir, dst_dir, n_pads):
    """A copy of the engine image in src_dir whose separable layers named in n_pads (scope suffix -> packed output columns) claim more
    packed columns than they have outputs.  The columns beyond cout read other weights of the image and are never stored, so the
    layer's outputs are those of the original record; only the kernel's column split differs."""
    blob = bytearray(open(os.path.join(src_dir, "mi355x.bin"), "rb").read())
    hdr = struct.unpack_from("<10I6f6Q12I", blob, 0)
    n_ops, ops_off = hdr[7], hdr[17]
    done = set()
    for i in range(n_ops):
        off = ops_off + engine.OP_RECORD_BYTES * i
        kind = struct.unpack_from("<i", blob, off)[0]
        name = struct.unpack_from("64s", blob, off + OP_NAME_OFFSET)[0].split(b"\0")[0].decode()
        for suffix, n_pad in n_pads.items():
            if kind == arch.OP_DWSEP and name.endswith("/" + suffix):
                struct.pack_into("<i", blob, off + 72, n_pad)
                done.add(suffix)
    assert done == set(n_pads), done
    os.makedirs(dst_dir, exist_ok=True)
    with open(os.path.join(dst_dir, "mi355x.bin"), "wb") as f:
        f.write(bytes(blob))
    return dst_dir


OP_NAME_OFFSET = engine.OP_RECORD_BYTES - 64


@pytest.mark.parametrize("n_pads", [
    {"Conv2d_1": 128, "Conv2d_2": 192, "Conv2d_5": 320},     # wz_k_dwsep<4, 2>, <2, 1>, <1, 1> at every batch
    {"Conv2d_2": 256, "Conv2d_3": 384, "Conv2d_4": 448, "Conv2d_6": 768},   # <2, 2> -> <2, 4> from batch 2 on; <1, 2>; <1, 1>; <1, 2> -> <1, 4>
], ids=["odd_groups", "wide_slices"])
def test_padded_column_groups_load_and_run_at_every_batch(v1_dirs, batch_frames, tmp_path, n_pads):
    """A separable layer whose packed columns are whole 64-column groups in a number that is not a power of two (192, 320, 384, 448)
    is accepted at load and then runs at batches 1 .. 8 -- the column split the launcher picks depends on the batch, and every split
    it can pick exists.  The rows equal those of the original image bit for bit at every batch."""
    path = _patched_image(v1_dirs["p16"], str(tmp_path / "patched"), n_pads)
    e_ref = conftest.make_engine(v1_dirs["p16"], max_batch=8)
    e_pad = conftest.make_engine(path, max_batch=8)
    try:
        for n in range(1, 9):
            fr = batch_frames[:n]
            ref = [np.zeros(100, ROW_DTYPE) for _ in fr]
            got = [np.zeros(100, ROW_DTYPE) for _ in fr]
            e_ref.detect_batch(fr, ref)
            e_pad.detect_batch(fr, got)
            for i, (g, r) in enumerate(zip(got, ref)):
                assert g.tobytes() == r.tobytes(), (n, i)
    finally:
        e_pad.close()
        e_ref.close()


def test_uncovered_separable_layer_refused_at_load(v1_dirs, tmp_path):
    """A WZ_OP_DWSEP record whose shape the kernel does not cover (here: 96 packed output columns, not a whole 64-column group) is
    refused by wz_create, naming the op -- never later as a run-time format error."""
    blob = bytearray(open(os.path.join(v1_dirs["p16"], "mi355x.bin"), "rb").read())
    hdr = struct.unpack_from("<10I6f6Q12I", blob, 0)
    n_ops, ops_off = hdr[7], hdr[17]
    for i in range(n_ops):
        off = ops_off + engine.OP_RECORD_BYTES * i
        kind, cout, n_pad = struct.unpack_from("<i", blob, off)[0], struct.unpack_from("<i", blob, off + 20)[0], \
            struct.unpack_from("<i", blob, off + 72)[0]
        if kind == arch.OP_DWSEP and cout == 64:
            assert n_pad == 64
            struct.pack_into("<i", blob, off + 72, 96)
            break
    else:
        pytest.fail("no 64-column separable layer")
    (tmp_path / "mi355x.bin").write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="Conv2d_1.*no depthwise-separable kernel"):   # (WZ_EFORMAT)
        conftest.make_engine(str(tmp_path), max_batch=2)

"""SSD-Inception-v2 on the CPU: the program (watsor_amd/inception.py), the builder and importer (watsor_amd/engine.py), the oracle's
pool semantics (tests/inception_v2_oracle.py) and the `-p 16` precision decision (the CPU emulation of that engine)."""
import json
import os
import struct

import numpy as np
import pytest

from watsor_amd import arch, engine, inception
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_weights

SEED = 1234


@pytest.fixture(scope="module")
def inc_weights():
    return synthetic_inception_v2(SEED)


@pytest.fixture(scope="module")
def inc_blob(inc_weights):
    return engine.build_engine(inc_weights, 16)


def parse_ops(blob):
    h = struct.unpack_from("<10I6f6Q12I", blob, 0)
    n_tensors, n_ops, tensors_off, ops_off = h[6], h[7], h[16], h[17]
    tensors = []
    for i in range(n_tensors):
        t = struct.unpack_from("<5i44s", blob, tensors_off + 64 * i)
        tensors.append(dict(h=t[0], w=t[1], c=t[2], slot=t[3], flags=t[4], name=t[5].split(b"\0")[0].decode()))
    ops = []
    for i in range(n_ops):
        o = struct.unpack_from("<20i2q8i8q64s", blob, ops_off + engine.OP_RECORD_BYTES * i)
        ops.append(dict(kind=o[0], src=o[1], dst=o[2], cin=o[4], cout=o[5], k=o[6], stride=o[7], hout=o[10], wout=o[11],
                        n_pad=o[18], kc=o[19], w_off=o[20], b_off=o[21], dst_coff=o[23], dst_c=o[24], flags=o[36],
                        name=o[38].split(b"\0")[0].decode()))
    return dict(version=h[1], precision=h[2], anchors=h[5], weights_off=h[19]), tensors, ops


def test_program_shapes_and_anchors(inc_weights):
    p = inception.build()
    maps = {"Conv2d_1a_7x7": (150, 64), "MaxPool_2a_3x3": (75, 64), "Conv2d_2b_1x1": (75, 64), "Conv2d_2c_3x3": (75, 192),
            "MaxPool_3a_3x3": (38, 192), "Mixed_3b": (38, 256), "Mixed_3c": (38, 320), "Mixed_4a": (19, 576), "Mixed_4b": (19, 576),
            "Mixed_4c": (19, 576), "Mixed_4d": (19, 576), "Mixed_4e": (19, 576), "Mixed_5a": (10, 1024), "Mixed_5b": (10, 1024),
            "Mixed_5c": (10, 1024)}
    for name, (hw, c) in maps.items():
        t = p.tensors[name]
        assert (t.h, t.w, t.c) == (hw, hw, c), name
    assert [(n, g, a) for n, g, a in p.feature_maps] == [
        ("Mixed_4c", 19, 3), ("Mixed_5c", 10, 6), ("Mixed_5c_2_Conv2d_2_3x3_s2_512", 5, 6), ("Mixed_5c_2_Conv2d_3_3x3_s2_256", 3, 6),
        ("Mixed_5c_2_Conv2d_4_3x3_s2_256", 2, 6), ("Mixed_5c_2_Conv2d_5_3x3_s2_128", 1, 6)]
    assert p.num_anchors == 1917
    assert [op.anchor_offset for op in p.ops if op.out_mode == arch.OUT_HEAD] == [0, 1083, 1683, 1833, 1887, 1911]
    shapes = p.variable_shapes()
    assert shapes == {k: tuple(v.shape) for k, v in inc_weights.items()}
    assert shapes["FeatureExtractor/InceptionV2/Conv2d_1a_7x7/depthwise_weights"] == (7, 7, 3, 8)
    assert shapes["FeatureExtractor/InceptionV2/Conv2d_1a_7x7/pointwise_weights"] == (1, 1, 24, 64)
    assert all(k.startswith("FeatureExtractor/InceptionV2/") or k.startswith("BoxPredictor_") for k in shapes)


def test_macs_per_frame():
    # the folded dense stem (150 x 150 x 64 x 147) included, pools none: ~2.6x MobileNet-v2's 1.9 G
    assert inception.macs_per_frame() == 4_948_529_984


def test_stem_fold_equals_depthwise_then_pointwise():
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(5)
    dw = rng.standard_normal((7, 7, 3, 8))
    pw = rng.standard_normal((1, 1, 24, 64))
    x = torch.from_numpy(rng.standard_normal((2, 3, 23, 21)))
    op = inception.build().ops[0]
    dense = engine.fold_stem7({op.scope + "/depthwise_weights": dw, op.scope + "/pointwise_weights": pw}, op)
    assert dense.shape == (7, 7, 3, 64) and dense.dtype == np.float64
    d = F.conv2d(x, torch.from_numpy(dw.transpose(2, 3, 0, 1).reshape(24, 1, 7, 7)), stride=2, groups=3)   # channel c*8+m
    two = F.conv2d(d, torch.from_numpy(pw.transpose(3, 2, 0, 1)))
    one = F.conv2d(x, torch.from_numpy(dense.transpose(3, 2, 0, 1)), stride=2)
    np.testing.assert_allclose(one.numpy(), two.numpy(), rtol=1e-12, atol=1e-11)


def test_oracle_pool_semantics():
    import torch
    from inception_v2_oracle import avg_pool_same, max_pool_same
    x = torch.arange(1, 26, dtype=torch.float32).reshape(1, 1, 5, 5)
    a = avg_pool_same(x, 1)[0, 0]
    assert float(a[0, 0]) == (1 + 2 + 6 + 7) / 4.0                       # corner: four in-image taps
    assert float(a[0, 2]) == (2 + 3 + 4 + 7 + 8 + 9) / 6.0               # edge: six
    assert float(a[2, 2]) == float(x[0, 0, 1:4, 1:4].mean())              # inside: nine
    neg = -torch.arange(1, 26, dtype=torch.float32).reshape(1, 1, 5, 5)
    m = max_pool_same(neg, 1)[0, 0]
    assert float(m[0, 0]) == -1.0 and float(m[4, 4]) == -19.0             # the zero padding never wins
    m2 = max_pool_same(neg, 2)[0, 0]
    assert tuple(m2.shape) == (3, 3) and float(m2[2, 2]) == -19.0


def _live_ranges(prog, names):
    first, last = {}, {}
    for i, op in enumerate(prog.ops):
        for n in (op.src, op.res):
            if n:
                last[n] = i
        if op.out_mode == arch.OUT_ACT:
            first.setdefault(op.dst, i)
    first["input"] = -1
    return {n: (first[n], last.get(n, first[n])) for n in names}


def test_slots_never_alias_live_tensors():
    prog = inception.build()
    names = ["input"] + list(dict.fromkeys(op.dst for op in prog.ops if op.out_mode == arch.OUT_ACT))
    slots = engine.assign_slots(prog, names)
    rng = _live_ranges(prog, names)
    assert all(s >= 0 for s in slots)
    for i, a in enumerate(names):
        for j, b in enumerate(names[:i]):
            (a0, a1), (b0, b1) = rng[a], rng[b]
            if a0 <= b1 and b0 <= a1:
                assert slots[i] != slots[j], (a, b)
    # a concat tensor is written by each branch; none of those ops reads a tensor in its slot
    writers = inception.tensor_writers(prog)
    slot = dict(zip(names, slots))
    for t, ops in writers.items():
        for i in ops:
            assert slot[prog.ops[i].src] != slot[t], (t, prog.ops[i].scope)
    assert len(writers["Mixed_3b"]) == 4 and len(writers["Mixed_4a"]) == 3


def test_engine_records_and_packing(inc_weights, inc_blob):
    hdr, tensors, ops = parse_ops(inc_blob)
    assert hdr["version"] == engine.FORMAT_VERSION == 12 and hdr["anchors"] == 1917
    prog = inception.build()
    assert len(ops) == len(prog.ops)
    tidx = {t["name"]: i for i, t in enumerate(tensors)}
    for o, op in zip(ops, prog.ops):
        assert o["kind"] == op.kind and o["name"] == op.scope
        if op.out_mode == arch.OUT_ACT:
            assert (o["dst_coff"], o["dst_c"]) == (op.coff, op.cdst)
            assert o["dst_coff"] + o["cout"] <= tensors[o["dst"]]["c"]
            if op.cdst:
                assert tensors[o["dst"]]["c"] == op.cdst == tensors[tidx[op.dst]]["c"]
        if op.kind == arch.OP_POOL:
            assert o["flags"] == (0 if op.pool_max else engine.POOL_AVG)
    # the slices of a module tile its channels exactly, in branch order
    for mod in ("Mixed_3b", "Mixed_4a", "Mixed_5c"):
        sl = sorted((o["dst_coff"], o["cout"]) for o in ops if o["dst"] == tidx[mod])
        assert sl[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(sl, sl[1:])) and sl[-1][0] + sl[-1][1] == tensors[tidx[mod]]["c"]
    # packed conv fragments round-trip: a sliced conv's weights are the folded fp16 weights in the MFMA order
    op_i = next(i for i, op in enumerate(prog.ops) if op.scope.endswith("Mixed_4c/Branch_2/Conv2d_0c_3x3"))
    o, op = ops[op_i], prog.ops[op_i]
    w, _ = engine.fold_batch_norm(inc_weights, op)
    taps = 9
    n = o["n_pad"] // 16 * taps * o["kc"] * 64 * 8
    packed = np.frombuffer(inc_blob, np.float16, n, hdr["weights_off"] + o["w_off"]).reshape(o["n_pad"] // 16, taps, o["kc"], 4, 16, 8)
    un = packed.transpose(1, 2, 3, 5, 0, 4).reshape(taps, o["kc"] * 32, o["n_pad"])[:, :op.cin, :op.cout]
    np.testing.assert_array_equal(un, w.reshape(taps, op.cin, op.cout).astype(np.float32).astype(np.float16))
    # the stem: K = tap * 4 + c in seven 32-row chunks
    st = ops[0]
    assert st["kind"] == arch.OP_STEM7 and st["kc"] == 7 and st["n_pad"] == 64
    dense, _ = engine.fold_batch_norm(inc_weights, prog.ops[0])
    packed = np.frombuffer(inc_blob, np.float16, 4 * 7 * 64 * 8, hdr["weights_off"] + st["w_off"]).reshape(4, 1, 7, 4, 16, 8)
    rows = packed.transpose(1, 2, 3, 5, 0, 4).reshape(224, 64)
    for t in (0, 1, 24, 48):
        np.testing.assert_array_equal(rows[t * 4:t * 4 + 3], dense[t // 7, t % 7].astype(np.float32).astype(np.float16))
        assert not rows[t * 4 + 3].any()
    assert not rows[196:].any()


def test_frozen_graph_gives_the_same_engine(tmp_path, inc_weights, inc_blob):
    pytest.importorskip("google.protobuf")
    from pb_writer import write_frozen_graph
    path = str(tmp_path / "frozen_inference_graph.pb")
    write_frozen_graph(path, inc_weights)
    w, settings = engine.load_model(path)
    assert engine.detect_family(w) == "InceptionV2"
    post, options = engine.apply_graph_settings(settings, 300, 300, None, None)
    assert engine.build_engine(w, 16, post=post, options=options) == inc_blob


def test_family_detection_and_refusals(tmp_path, inc_weights):
    mb = synthetic_weights(SEED)
    assert engine.detect_family(mb) == "MobilenetV2" and engine.detect_family(inc_weights) == "InceptionV2"
    v1 = {k.replace("MobilenetV2", "MobilenetV1"): v for k, v in mb.items()}
    with pytest.raises(ValueError, match="MobilenetV1.*SSD-MobileNet-v2.*SSD-Inception-v2"):
        engine.build_engine(v1)
    np.savez(tmp_path / "v1.npz", **v1)
    with pytest.raises(ValueError, match="MobilenetV1"):
        engine.main(["-i", str(tmp_path / "v1.npz"), "-o", str(tmp_path / "x.bin")])
    for flags in (["--robust", "on"], ["--plain-fp16"]):
        with pytest.raises(ValueError, match="SSD-Inception-v2"):
            engine.main(["-i", "synthetic_inception_v2", "-o", str(tmp_path / "y.bin")] + flags)
    with pytest.raises(ValueError):
        engine.build_engine(inc_weights, robust=True)
    bad = dict(inc_weights)
    name = "FeatureExtractor/InceptionV2/Mixed_4c/Branch_1/Conv2d_0b_3x3/weights"
    bad[name] = np.zeros((3, 3, 96, 129), np.float32)
    with pytest.raises(ValueError, match="Mixed_4c/Branch_1/Conv2d_0b_3x3"):
        engine.build_engine(bad)


def test_cli_builds_both_precisions_and_reads_head_kernel_size(tmp_path, inc_weights, capsys):
    for p in ("16", "32"):
        out = tmp_path / ("p%s.bin" % p)
        assert engine.main(["-i", "synthetic_inception_v2:7", "-p", p, "-o", str(out), "--robust", "auto"]) == 0
        hdr, _, ops = parse_ops(out.read_bytes())
        assert hdr["precision"] == int(p) and ops[0]["kind"] == arch.OP_STEM7
    assert "SSD-Inception-v2" in capsys.readouterr().out
    # 1x1 box predictors (a config with kernel_size 1): the heads follow the weights
    w = dict(inc_weights)
    for i in range(6):
        for sub in ("BoxEncodingPredictor", "ClassPredictor"):
            k = "BoxPredictor_%d/%s/weights" % (i, sub)
            w[k] = np.ascontiguousarray(w[k][1:2, 1:2])
    _, _, ops = parse_ops(engine.build_engine(w, 16))
    assert [o["k"] for o in ops if o["name"].startswith("BoxPredictor_")] == [1] * 6


def test_fp16_emulation_within_the_bar(inc_weights):
    """The `-p 16` engine emulated on the CPU (fp16 folded weights, fp16 storage of every stored tensor, fp32 sums, fp16 input)
    against the fp32 oracle on 4 frames: max score deviation <= 7e-4, so the plain fp16 program ships (recorded in
    profiles/inception_fp16_emulation.json by tools/inception_precision.py)."""
    from inception_v2_oracle import InceptionOracleNet
    from oracle import preprocess as pre
    from oracle.postprocess import sigmoid
    frames = [synthetic_frame(640, 480, s) for s in (1, 2, 3, 4)]
    x = np.stack([pre.preprocess(f, 300) for f in frames])
    _, lg, _ = InceptionOracleNet(inc_weights).forward(x)
    _, lg16, _ = InceptionOracleNet(inc_weights, emulate16=True).forward(x)
    dev = float(np.abs(sigmoid(lg) - sigmoid(lg16)).max())
    assert dev <= 7e-4, dev
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "inception_fp16_emulation.json")) as f:
        rec = json.load(f)
    assert rec["decision"] == "plain fp16" and rec["max_score_dev"] <= 7e-4

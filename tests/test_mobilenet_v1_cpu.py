"""SSD-MobileNet-v1 on the CPU: the program (watsor_amd/mobilenet_v1.py), the builder and importer (watsor_amd/engine.py), the fused
separable-layer records and the `-p 16` precision decision (the CPU emulation of that engine, tests/mobilenet_v1_oracle.py)."""
import json
import os
import struct

import numpy as np
import pytest

from watsor_amd import arch, engine, mobilenet_v1
from watsor_amd.synth import synthetic_frame, synthetic_inception_v2, synthetic_mobilenet_v1, synthetic_weights

SEED = 1234
FE = "FeatureExtractor/MobilenetV1/"


@pytest.fixture(scope="module")
def v1_weights():
    return synthetic_mobilenet_v1(SEED)


@pytest.fixture(scope="module")
def v1_blob(v1_weights):
    return engine.build_engine(v1_weights, 16)


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
        ops.append(dict(kind=o[0], src=o[1], dst=o[2], res=o[3], cin=o[4], cout=o[5], k=o[6], stride=o[7], hin=o[8], win=o[9],
                        hout=o[10], wout=o[11], pad_t=o[12], pad_l=o[13], act=o[14], n_pad=o[18], kc=o[19], w_off=o[20], b_off=o[21],
                        cmid=o[23], cin0=o[24], wd_off=o[32], bd_off=o[33], flags=o[36], name=o[38].split(b"\0")[0].decode()))
    return dict(version=h[1], precision=h[2], anchors=h[5], weights_off=h[19], hp_blocks=h[23]), tensors, ops


def test_program_shapes_and_anchors(v1_weights):
    p = mobilenet_v1.build()
    maps = {"Conv2d_0": (150, 32), "Conv2d_1_pointwise": (150, 64), "Conv2d_2_pointwise": (75, 128), "Conv2d_3_pointwise": (75, 128),
            "Conv2d_4_pointwise": (38, 256), "Conv2d_5_pointwise": (38, 256), "Conv2d_6_pointwise": (19, 512),
            "Conv2d_11_pointwise": (19, 512), "Conv2d_12_pointwise": (10, 1024), "Conv2d_13_pointwise": (10, 1024)}
    for name, (hw, c) in maps.items():
        t = p.tensors[name]
        assert (t.h, t.w, t.c) == (hw, hw, c), name
    assert [(n, g, a) for n, g, a in p.feature_maps] == [
        ("Conv2d_11_pointwise", 19, 3), ("Conv2d_13_pointwise", 10, 6), ("Conv2d_13_pointwise_2_Conv2d_2_3x3_s2_512", 5, 6),
        ("Conv2d_13_pointwise_2_Conv2d_3_3x3_s2_256", 3, 6), ("Conv2d_13_pointwise_2_Conv2d_4_3x3_s2_256", 2, 6),
        ("Conv2d_13_pointwise_2_Conv2d_5_3x3_s2_128", 1, 6)]
    assert p.num_anchors == 1917
    assert [op.anchor_offset for op in p.ops if op.out_mode == arch.OUT_HEAD] == [0, 1083, 1683, 1833, 1887, 1911]
    assert [op.kind for op in p.ops[:14]] == [arch.OP_STEM] + [arch.OP_DWSEP] * 13
    unf = mobilenet_v1.build(fuse=False)
    assert [op.kind for op in unf.ops[:27]] == [arch.OP_STEM] + [arch.OP_DW, arch.OP_CONV] * 13
    assert unf.tensors["Conv2d_12_depthwise"].h == 10 and unf.tensors["Conv2d_13_depthwise"].c == 1024


def test_macs_per_frame():
    # an independent count: stem, 13 x (depthwise 9 C + pointwise C x C'), extras, the six heads at 3 x 3
    maps = [150, 150, 75, 75, 38, 38, 19, 19, 19, 19, 19, 19, 10, 10]      # output map of Conv2d_0 .. Conv2d_13
    chans = [32, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024]
    body = 150 * 150 * 32 * 27
    pointwise = 0
    for i in range(1, 14):
        body += maps[i] ** 2 * chans[i - 1] * 9
        pointwise += maps[i] ** 2 * chans[i - 1] * chans[i]
    extras = 0
    cin, hw = 1024, 10
    for d1, d2 in ((256, 512), (128, 256), (128, 256), (64, 128)):
        extras += hw * hw * cin * d1
        hw = (hw + 1) // 2
        extras += hw * hw * 9 * d1 * d2
        cin = d2
    heads = sum(g * g * 9 * c * a * 95 for g, c, a in ((19, 512, 3), (10, 1024, 6), (5, 512, 6), (3, 256, 6), (2, 256, 6), (1, 128, 6)))
    assert 0.95e9 < pointwise < 1.05e9                                     # the 13 pointwise layers: ~1.0 G
    assert mobilenet_v1.macs_per_frame() == body + pointwise + extras + heads == 2_199_617_728
    assert mobilenet_v1.macs_per_frame(mobilenet_v1.build(fuse=False)) == mobilenet_v1.macs_per_frame()


def test_variable_shapes_and_refusal_by_name(v1_weights):
    shapes = mobilenet_v1.build().variable_shapes()
    assert shapes == {k: tuple(v.shape) for k, v in v1_weights.items()}
    assert shapes == mobilenet_v1.build(fuse=False).variable_shapes()
    assert shapes[FE + "Conv2d_0/weights"] == (3, 3, 3, 32)
    assert shapes[FE + "Conv2d_7_depthwise/depthwise_weights"] == (3, 3, 512, 1)
    assert shapes[FE + "Conv2d_13_pointwise/weights"] == (1, 1, 1024, 1024)
    assert shapes[FE + "Conv2d_13_pointwise_1_Conv2d_2_1x1_256/weights"] == (1, 1, 1024, 256)
    assert shapes[FE + "Conv2d_13_pointwise_2_Conv2d_5_3x3_s2_128/weights"] == (3, 3, 64, 128)
    assert shapes["BoxPredictor_0/ClassPredictor/weights"] == (3, 3, 512, 273)
    assert all(k.startswith(FE) or k.startswith("BoxPredictor_") for k in shapes)
    bad = dict(v1_weights)
    name = FE + "Conv2d_9_pointwise/weights"
    bad[name] = np.zeros((1, 1, 512, 520), np.float32)
    with pytest.raises(ValueError, match="Conv2d_9_pointwise"):
        engine.build_engine(bad)


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


@pytest.mark.parametrize("fuse", [True, False])
def test_slots_never_alias_live_tensors(fuse):
    prog = mobilenet_v1.build(fuse=fuse)
    names = ["input"] + [op.dst for op in prog.ops if op.out_mode == arch.OUT_ACT]
    slots = engine.assign_slots(prog, names)
    rng = _live_ranges(prog, names)
    assert all(s >= 0 for s in slots)
    for i, a in enumerate(names):
        for j, b in enumerate(names[:i]):
            (a0, a1), (b0, b1) = rng[a], rng[b]
            if a0 <= b1 and b0 <= a1:
                assert slots[i] != slots[j], (a, b)
    slot = dict(zip(names, slots))
    for op in prog.ops:
        if op.out_mode == arch.OUT_ACT:
            assert slot[op.src] != slot[op.dst], op.scope


def test_fused_records_and_packing(v1_weights, v1_blob):
    hdr, tensors, ops = parse_ops(v1_blob)
    assert hdr["version"] == engine.FORMAT_VERSION == 12 and hdr["anchors"] == 1917 and hdr["precision"] == 16 and hdr["hp_blocks"] == 0
    prog = mobilenet_v1.build()
    assert len(ops) == len(prog.ops) == 1 + 13 + 8 + 6
    tidx = {t["name"]: i for i, t in enumerate(tensors)}
    assert not any(n.endswith("_depthwise") for n in tidx)
    fused = [(o, op) for o, op in zip(ops, prog.ops) if op.kind == arch.OP_DWSEP]
    assert len(fused) == 13 and all(o["kind"] == 7 == arch.OP_DWSEP for o, _ in fused)
    for o, op in fused:
        dw, pw = op.parts
        assert (dw.kind, pw.kind) == (arch.OP_DW, arch.OP_CONV) and dw.scope.endswith("_depthwise") and pw.scope.endswith("_pointwise")
        assert o["name"] == op.scope and o["cin"] == dw.cin == pw.cin and o["cout"] == pw.cout and (o["k"], o["stride"]) == (3, dw.stride)
        assert (o["hin"], o["win"], o["hout"], o["wout"]) == (dw.hin, dw.win, pw.hout, pw.wout) and (pw.hin, pw.hout) == (dw.hout, dw.hout)
        assert (o["pad_t"], o["pad_l"]) == (dw.pad_t, dw.pad_l) and o["act"] == arch.ACT_RELU6 and o["res"] == -1
        assert o["kc"] == o["cin"] // 32 and o["n_pad"] == o["cout"] and o["n_pad"] % 64 == 0
        assert o["cmid"] == 0 and o["cin0"] == 0 and o["flags"] == 0
        assert tensors[o["src"]]["c"] == o["cin"] and tensors[o["dst"]]["name"] == pw.dst
        assert len({o["wd_off"], o["bd_off"], o["w_off"], o["b_off"]}) == 4 and all(o[k] % 256 == 0 for k in ("wd_off", "bd_off", "w_off", "b_off"))
        # depthwise: the WZ_OP_DW layout (half w[9][C], float bias[C]) at wd_off / bd_off
        wd, bd = engine.fold_batch_norm(v1_weights, dw)
        got = np.frombuffer(v1_blob, np.float16, 9 * dw.cin, hdr["weights_off"] + o["wd_off"]).reshape(9, dw.cin)
        np.testing.assert_array_equal(got, wd.reshape(9, dw.cin).astype(np.float16))
        np.testing.assert_array_equal(np.frombuffer(v1_blob, np.float32, dw.cin, hdr["weights_off"] + o["bd_off"]), bd.astype(np.float32))
    # pointwise: the WZ_OP_CONV layout with one tap at w_off / b_off -- round-trip one layer's fragments
    o, op = fused[8]
    pw = op.parts[1]
    w, b = engine.fold_batch_norm(v1_weights, pw)
    n = o["n_pad"] // 16 * o["kc"] * 64 * 8
    packed = np.frombuffer(v1_blob, np.float16, n, hdr["weights_off"] + o["w_off"]).reshape(o["n_pad"] // 16, 1, o["kc"], 4, 16, 8)
    un = packed.transpose(1, 2, 3, 5, 0, 4).reshape(o["kc"] * 32, o["n_pad"])[:pw.cin, :pw.cout]
    np.testing.assert_array_equal(un, w.reshape(pw.cin, pw.cout).astype(np.float32).astype(np.float16))
    np.testing.assert_array_equal(np.frombuffer(v1_blob, np.float32, pw.cout, hdr["weights_off"] + o["b_off"]), b.astype(np.float32))


def test_unfused_and_p32_programs(v1_weights):
    for p, fuse in ((16, False), (32, True)):
        hdr, tensors, ops = parse_ops(engine.build_engine(v1_weights, p, fuse=fuse))
        assert hdr["precision"] == p and len(ops) == 1 + 26 + 8 + 6
        assert arch.OP_DWSEP not in [o["kind"] for o in ops]
        assert (tensors[0]["flags"] == 1) == (p == 32)                     # -p 32: the input as a hi + lo pair
        assert [o["kind"] for o in ops[:3]] == [arch.OP_STEM, arch.OP_DW, arch.OP_CONV]


def test_frozen_graph_gives_the_same_engine(tmp_path, v1_weights, v1_blob):
    pytest.importorskip("google.protobuf")
    from pb_writer import write_frozen_graph
    path = str(tmp_path / "frozen_inference_graph.pb")
    write_frozen_graph(path, v1_weights)
    w, settings = engine.load_model(path)
    assert engine.detect_family(w) == "MobilenetV1"
    post, options = engine.apply_graph_settings(settings, 300, 300, None, None)
    assert engine.build_engine(w, 16, post=post, options=options) == v1_blob
    np.savez(tmp_path / "v1.npz", **v1_weights)
    assert engine.build_engine(engine.load_weights(str(tmp_path / "v1.npz")), 16) == v1_blob
    assert engine.build_engine(engine.load_weights("synthetic_mobilenet_v1:%d" % SEED), 16) == v1_blob


def test_family_detection_and_refusals(tmp_path, v1_weights):
    mb = synthetic_weights(SEED)
    inc = synthetic_inception_v2(SEED)
    assert [engine.detect_family(w) for w in (mb, inc, v1_weights)] == ["MobilenetV2", "InceptionV2", "MobilenetV1"]
    assert list(engine.FAMILIES) == ["MobilenetV2", "InceptionV2", "MobilenetV1"]
    # MobileNet-v2 variables under the MobilenetV1 scope are not SSD-MobileNet-v1's: a ValueError before anything reads them
    renamed = {k.replace("MobilenetV2", "MobilenetV1"): v for k, v in mb.items()}
    for call in (engine.detect_family, engine.build_engine, engine.channel_spread_decades):
        with pytest.raises(ValueError, match="MobilenetV1.*not SSD-MobileNet-v1's.*SSD-MobileNet-v2.*SSD-Inception-v2"):
            call(renamed)
    for flags in (["--robust", "on"], ["--plain-fp16"]):
        with pytest.raises(ValueError, match="SSD-MobileNet-v1"):
            engine.main(["-i", "synthetic_mobilenet_v1", "-o", str(tmp_path / "y.bin")] + flags)
    for kw in (dict(robust=True), dict(hp_upto=3), dict(conv1_split=True)):
        with pytest.raises(ValueError, match="SSD-MobileNet-v1"):
            engine.build_engine(v1_weights, **kw)
    partial = {k: v for k, v in v1_weights.items() if not k.startswith(FE + "Conv2d_7_depthwise/")}
    with pytest.raises(ValueError, match="not SSD-MobileNet-v1's \\(5 of its variables missing, e.g. %sConv2d_7_depthwise/" % FE):
        engine.build_engine(partial)
    other = dict(v1_weights)
    other["FeatureExtractor/ResnetV1_50/conv1/weights"] = np.zeros((7, 7, 3, 64), np.float32)
    with pytest.raises(ValueError, match="MobilenetV1 \\+ ResnetV1_50"):
        engine.build_engine(other)
    assert 0.1 < engine.channel_spread_decades(v1_weights) < engine.SPREAD_VALIDATED_DECADES


def test_other_float_constants_under_the_scope_are_ignored(v1_weights, v1_blob):
    """A frozen graph holds every float constant under the scope, not only weights (an unfused BatchNorm's epsilon, for one): those
    the program does not read change nothing, as for the other two networks."""
    w = dict(v1_weights)
    w[FE + "Conv2d_3_pointwise/BatchNorm/batchnorm/add/y"] = np.array(1e-3, np.float32)
    w[FE + "Conv2d_13_pointwise_2_Conv2d_2_3x3_s2_512/BatchNorm/batchnorm/add/y"] = np.array(1e-3, np.float32)
    assert engine.detect_family(w) == "MobilenetV1"
    assert engine.build_engine(w, 16) == v1_blob


def test_cli_builds_both_precisions(tmp_path, v1_weights, capsys):
    for p in ("16", "32"):
        out = tmp_path / ("p%s.bin" % p)
        assert engine.main(["-i", "synthetic_mobilenet_v1:7", "-p", p, "-o", str(out), "--robust", "auto"]) == 0
        hdr, _, ops = parse_ops(out.read_bytes())
        assert hdr["precision"] == int(p) and ops[0]["kind"] == arch.OP_STEM
        assert (ops[1]["kind"] == arch.OP_DWSEP) == (p == "16")
    text = capsys.readouterr().out
    assert "Network: SSD-MobileNet-v1 (FeatureExtractor/MobilenetV1/)" in text
    np.savez(tmp_path / "v1.npz", **v1_weights)
    assert engine.main(["-i", str(tmp_path / "v1.npz"), "-o", str(tmp_path / "npz.bin")]) == 0
    assert (tmp_path / "npz.bin").read_bytes() == engine.build_engine(v1_weights, 16)


def test_fp16_emulation_within_the_bar(v1_weights):
    """The `-p 16` engine emulated on the CPU (fp16 folded weights, fp16 storage of every stored tensor -- the depthwise outputs
    included --, fp32 sums, fp16 input) against the fp32 oracle on 4 frames: max score deviation <= 7e-4, so the plain fp16 program
    ships (recorded in profiles/mobilenet_v1_fp16_emulation.json by tools/inception_precision.py --network mobilenet_v1)."""
    from mobilenet_v1_oracle import MobilenetV1OracleNet
    from oracle import preprocess as pre
    from oracle.postprocess import sigmoid
    frames = [synthetic_frame(640, 480, s) for s in (1, 2, 3, 4)]
    x = np.stack([pre.preprocess(f, 300) for f in frames])
    _, lg, _ = MobilenetV1OracleNet(v1_weights).forward(x)
    _, lg16, _ = MobilenetV1OracleNet(v1_weights, emulate16=True).forward(x)
    dev = float(np.abs(sigmoid(lg) - sigmoid(lg16)).max())
    assert dev <= 7e-4, dev
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "mobilenet_v1_fp16_emulation.json")) as f:
        rec = json.load(f)
    assert rec["decision"] == "plain fp16" and rec["max_score_dev"] <= 7e-4
    assert abs(rec["max_score_dev"] - dev) <= 1e-6

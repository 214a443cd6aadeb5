"""engine.assign_slots packs tensors whose lifetimes do not overlap into one HBM buffer.  The lifetimes that count are those of the
ENQUEUE (csrc/wz_network.hip), not of the program's list: an op runs at its index, except a head -- the heads' convolutions are
grouped launches of HeadPark::flush, after the last op, so a head's source is read at the END of the batch whatever the head's index.
`conflicts` replays a slot assignment against that order; every program the builder packs must pass it, with the slots it had before
the rule knew about the heads (number and sizes pinned below), and a toy program with an activation op between two heads -- where the
list order and the order of execution part -- shows that the replay sees the difference."""
import pytest

from watsor_amd import arch, engine, synth

SEED = 1234

# program -> (weights of watsor_amd.synth, build_engine's arguments, slot sizes in halves per frame)
PROGRAMS = {
    "default":              ("synthetic_weights", dict(), [720000, 720000, 207936, 12800, 2304, 1024, 128]),
    "robust":               ("synthetic_weights", dict(robust=True), [720000, 720000, 207936, 12800, 2304, 1024, 128]),
    "plain":                ("synthetic_weights", dict(hp_upto=-1), [360000, 360000, 207936, 12800, 2304, 1024, 128]),
    "unfused":              ("synthetic_weights", dict(fuse=False), [2160000, 810000, 810000, 128000, 2304, 1024, 128]),
    "stem_separate":        ("synthetic_weights", dict(fuse_stem=False), [360000, 720000, 32000, 12800, 2304, 1024, 128]),
    "fp32":                 ("synthetic_weights", dict(precision=32), [2160000, 810000, 810000, 128000, 2304, 1024, 128]),
    "inception_v2":         ("synthetic_inception_v2", dict(precision=16), [1080000, 1440000, 369664, 462080, 207936, 1024, 128]),
    "inception_v2_p32":     ("synthetic_inception_v2", dict(precision=32), [1080000, 1440000, 369664, 462080, 207936, 1024, 128]),
    "mobilenet_v1":         ("synthetic_mobilenet_v1", dict(precision=16, fuse=True), [1440000, 720000, 102400, 12800, 2304, 1024, 128]),
    "mobilenet_v1_unfused": ("synthetic_mobilenet_v1", dict(precision=16, fuse=False), [720000, 1440000, 102400, 12800, 2304, 1024, 128]),
    "mobilenet_v1_p32":     ("synthetic_mobilenet_v1", dict(precision=32), [720000, 1440000, 102400, 12800, 2304, 1024, 128]),
    "robust_no_float_form": ("synthetic_weights", dict(robust=True, float_form_upto=-1), [720000, 720000, 207936, 12800, 2304, 1024, 128]),
    "robust_float_form_12": ("synthetic_weights", dict(robust=True, float_form_upto=12), [720000, 720000, 207936, 12800, 2304, 1024, 128]),
    "robust_conv1_plain":   ("synthetic_weights", dict(robust=True, conv1_split=False), [720000, 720000, 207936, 12800, 2304, 1024, 128]),
    "tap_not_in_block":     ("synthetic_weights", dict(tap_in_block=False), [720000, 720000, 32000, 12800, 2304, 1024, 128]),
}


def tensor_size(prog, name):
    t = prog.tensors[name]
    return t.h * t.w * (4 if name == "input" else t.c) * (2 if t.hp else 1)


def lifetimes(prog, names):
    """name -> (first write, last access, every write) in the enqueue's order of execution: op i at time i, a head's read at
    time len(ops) (HeadPark::flush); the input is written at -1.  A concat tensor lives from its first writer."""
    end = len(prog.ops)
    writes = {n: [] for n in names}
    reads = {n: [] for n in names}
    writes["input"].append(-1)
    for i, op in enumerate(prog.ops):
        head = op.out_mode != arch.OUT_ACT
        for t in (op.src, op.res):
            if t:
                reads[t].append(end if head else i)
        if not head:
            for t in (op.dst, op.dst2):
                if t:
                    writes[t].append(i)
    return {n: (min(writes[n]), max(writes[n] + reads[n]), writes[n]) for n in names}


def conflicts(prog, names, slots):
    """Messages, one per pair (t, u) of tensors in one slot with a write of u between t's first write and t's last access (the ends
    included: an op may not write over what it reads, nor two of its outputs over each other)."""
    life = lifetimes(prog, names)
    out = []
    for a, t in enumerate(names):
        for b in range(a + 1, len(names)):
            u = names[b]
            if slots[a] != slots[b]:
                continue
            for x, y in ((t, u), (u, t)):
                first, last, _ = life[x]
                hit = [w for w in life[y][2] if first <= w <= last]
                if hit:
                    out.append("slot %d: %s (alive %d .. %d) is overwritten by %s at %s" % (slots[a], x, first, last, y, hit))
                    break
    return out


def heads_last_and_allocate_nothing(prog):
    """The fact the builders rely on, as messages: every head op sits behind every activation-producing op and has no tensor of its own."""
    heads = [i for i, op in enumerate(prog.ops) if op.out_mode != arch.OUT_ACT]
    out = []
    if not heads:
        out.append("no head ops")
    elif heads != list(range(len(prog.ops) - len(heads), len(prog.ops))):
        out.append("head ops at %s of %d ops: an activation-producing op runs behind a head" % (heads, len(prog.ops)))
    for i in heads:
        if prog.ops[i].dst2 or prog.ops[i].dst in prog.tensors:
            out.append("head op %d writes the tensor %s" % (i, prog.ops[i].dst2 or prog.ops[i].dst))
    return out


_weights = {}


def packed(name, monkeypatch):
    """(program, tensor names, slots) exactly as build_engine handed them to / got them from assign_slots"""
    source, kw, _ = PROGRAMS[name]
    if source not in _weights:
        _weights[source] = getattr(synth, source)(SEED)
    seen = []
    real = engine.assign_slots

    def spy(prog, names):
        slots = real(prog, names)
        seen.append((prog, list(names), list(slots)))
        return slots
    monkeypatch.setattr(engine, "assign_slots", spy)
    engine.build_engine(_weights[source], **kw)
    assert len(seen) == 1
    return seen[0]


@pytest.mark.parametrize("name", list(PROGRAMS))
def test_no_slot_is_overwritten_while_its_tensor_lives(name, monkeypatch):
    prog, names, slots = packed(name, monkeypatch)
    assert names[0] == "input" and len(set(names)) == len(names) == len(slots) and min(slots) == 0
    assert set(names) == {"input"} | {t for op in prog.ops if op.out_mode == arch.OUT_ACT for t in (op.dst, op.dst2) if t}
    assert conflicts(prog, names, slots) == []
    assert heads_last_and_allocate_nothing(prog) == []
    # sharing happens at all (the replay is not looking at one buffer per tensor) ...
    assert max(slots) + 1 < len(names)
    # ... and exactly as before the heads' sources lived to the end
    sizes = [0] * (max(slots) + 1)
    for t, s in zip(names, slots):
        sizes[s] = max(sizes[s], tensor_size(prog, t))
    assert sizes == PROGRAMS[name][2]


def toy_program():
    """input -> t1 -> t2 -> t3 with a head on t1 BETWEEN the ops that make t2 and t3, and a head on t3.  t1 and t3 have one size."""
    p = arch.Program(size=8)
    p.tensors = {"input": arch.Tensor("input", 8, 8, 3), "t1": arch.Tensor("t1", 4, 4, 16), "t2": arch.Tensor("t2", 4, 4, 32),
                 "t3": arch.Tensor("t3", 4, 4, 16)}

    def conv(src, dst, cin, cout, **kw):
        return arch.Op(arch.OP_CONV, dst, src, dst, cin, cout, 1, 1, arch.ACT_RELU6, True, **kw)
    p.ops = [conv("input", "t1", 3, 16), conv("t1", "t2", 16, 32), conv("t1", "head_0", 16, 8, out_mode=arch.OUT_HEAD),
             conv("t2", "t3", 32, 16), conv("t3", "head_1", 16, 8, out_mode=arch.OUT_HEAD)]
    return p, ["input", "t1", "t2", "t3"]


def test_an_activation_op_between_two_heads_is_flagged():
    prog, names = toy_program()
    assert heads_last_and_allocate_nothing(prog) != []
    # what releasing t1 at its head's INDEX gives: t3 takes t1's slot, and op 3 writes it before the parked head 0 has read t1
    by_index = [0, 1, 2, 1]
    msgs = conflicts(prog, names, by_index)
    assert len(msgs) == 1 and "t1" in msgs[0] and "t3" in msgs[0], msgs
    # the same assignment is fine for a program that runs in list order -- the replay's order is what flags it
    assert lifetimes(prog, names)["t1"][1] == len(prog.ops)
    # one buffer per tensor is always clean, and assign_slots keeps a head's source to the end
    assert conflicts(prog, names, [0, 1, 2, 3]) == []
    slots = engine.assign_slots(prog, names)
    assert conflicts(prog, names, slots) == []
    assert slots[names.index("t3")] != slots[names.index("t1")]
    assert slots[names.index("t2")] == slots[names.index("input")]          # (sharing still happens where it is safe)


def test_the_replay_sees_an_op_writing_over_its_own_source():
    prog, names = toy_program()
    assert any("t2" in m and "t1" in m for m in conflicts(prog, names, [0, 1, 1, 3]))

"""CPU restatement of HOW wz_k_tile_activity (csrc/k_gate.hip) walks one tile -- tests/gate_oracle.py states WHAT the answer is.  numpy
integers only, the 64 lanes of a wave as one array axis:

    tile_geometry(w, fmt, rect)                                   -> (offset, pitch, row_bytes, mode): csrc/wz_tiles.hip's gate_tile
    walk(frame, addr16, offset, pitch, row_bytes, tw, th, mode)   -> (uint16 [cell rows, cell columns], census of the paths taken)

`frame` holds the frame's bytes and `addr16` is the address of its first byte modulo 16; the tile's rows are `th` runs of `row_bytes`
bytes, `pitch` apart, the first `offset` bytes into the frame.  A wave owns one row and walks it in aligned 16-byte words, 64 a trip of
its loop, exactly as the kernel does: the row's `head`, its ragged first and last words, the split of a word between two cells at
`bnd`, the even / odd byte select, WZ_GATE_LOW10's per-byte shares, the m / e / tail / shuffle / carry63 scheme for three-byte pixels
and the load of the next trip's words one trip ahead.

Memory is modelled as what it is: 16-byte words at aligned addresses.  Word k of a row is the k-th aligned word from the one that
holds the row's first byte, and `head` only says which of its bytes belong to the row.  With the kernel's own `head` that is the
kernel's `rs + 16 k - head`; with a wrong one (defect "head_of_row0") the words stay where they are and their bytes are taken for
other bytes of the row -- what a load that drops the low address bits, or a head hoisted out of the row loop, would give.

`defect=` seeds one mistake the kernel could make:
    carry_never          carry63 is never updated: lane 0 of a later trip starts a straddling pixel from 0
    carry_lane62         carry63 is taken from lane 62
    prefetch_same_words  the prefetch loads word k instead of k + 64: the second trip sums the first trip's words again
    one_trip             the loop stops after its first trip
    guard_first_trip     the `k < words` guard of the LDS adds reads `k < 64`
    head_of_row0         every row uses row 0's head
All but the last live in trips beyond the first only (BEYOND_FIRST_TRIP): a row of at most 64 words cannot see them.
"""
import numpy as np

CELL = 16
LANES = 64
GRAY, YUYV, UYVY, RGB, BGR, LOW10 = range(6)          # csrc/wz_common.h: WZ_GATE_*
BEYOND_FIRST_TRIP = ("carry_never", "carry_lane62", "prefetch_same_words", "one_trip", "guard_first_trip")
DEFECTS = BEYOND_FIRST_TRIP + ("head_of_row0",)

_MODE_OF_BASE = {0: RGB, 6: BGR, 3: YUYV, 4: UYVY, 0x10: UYVY, 0x11: LOW10, 1: GRAY, 2: GRAY, 5: GRAY}
_J = np.arange(16, dtype=np.int64)


def tile_geometry(w: int, fmt: int, rect):
    """What the kernel reads of rectangle (x0, y0, tw, th) of a frame w pixels wide: the luma-bearing bytes of its rows.  A P010 word's
    top eight bits are its second byte (UYVY's odd bytes), a YUV420P10 word's are bits 2 .. 9 (LOW10)."""
    mode = _MODE_OF_BASE[fmt & 0xFF]
    bpp = 3 if mode in (RGB, BGR) else 1 if mode == GRAY else 2
    x0, y0, tw, _th = rect
    return (y0 * w + x0) * bpp, w * bpp, tw * bpp, mode


def new_census():
    return {"trips": set(),                   # (trips of a row, words in its last trip)
            "e_at_trip": set(),               # three-byte modes: e of lane 0 with base > 0
            "boundary_mod3": set(),           # ... and (64 * 16 * s - head) % 3 there
            "heads": set(),                   # head of every row
            "multi_trip_head_parity": set(),  # head & 1 of the rows with two or more trips
            "low10_split_at_trip": False,     # a LOW10 word's two bytes in the last word of one trip and the first of the next
            "two_cells": False,               # a word added to cell_a and to cell_a + 1
            "last_cell_cut": False,           # a word that reaches past its cell in the tile's last cell column
            "zero_sum_skipped": False,        # `if (sum_a)` held an add back
            "ragged_first": False, "ragged_last": False}


def merge_census(into, other):
    for key, val in other.items():
        into[key] = into[key] | val
    return into


def walk(frame, addr16: int, offset: int, pitch: int, row_bytes: int, tw: int, th: int, mode: int, defect=None):
    assert defect is None or defect in DEFECTS, defect
    data = np.asarray(frame, np.uint8).reshape(-1)
    addr16 &= 15
    mem = np.zeros(addr16 + data.size + 16 * (2 * LANES + 4), np.int64)      # zeros behind the frame: a defect may read past it
    mem[addr16:addr16 + data.size] = data
    cols, crows = -(-tw // CELL), -(-th // CELL)
    out = np.zeros((crows, cols), np.uint16)
    census = new_census()
    three = mode in (RGB, BGR)
    cell_shift = 4 if mode == GRAY else 5
    w_first, w_last = (77, 29) if mode == RGB else (29, 77)
    lanes = np.arange(LANES, dtype=np.int64)
    rb = row_bytes
    for strip in range(crows):
        cells = np.zeros(cols, np.int64)                                     # the strip's LDS
        for row in range(strip * CELL, min(th, (strip + 1) * CELL)):         # one wave each
            at = addr16 + offset + row * pitch                               # the row's first byte in `mem`
            aligned = at - (at & 15)
            head = (addr16 + offset) & 15 if defect == "head_of_row0" else at & 15
            words = (head + rb + 15) >> 4
            trips = -(-words // LANES)
            census["heads"].add(head)
            census["trips"].add((trips, words - LANES * (trips - 1)))
            if trips > 1:
                census["multi_trip_head_parity"].add(head & 1)

            def load(k):
                lo = k * 16 - head
                o = lo[:, None] + _J[None, :]
                inside = (o >= 0) & (o < rb) & (k < words)[:, None]          # no byte outside [row, row + row_bytes)
                census["ragged_first"] |= bool(((lo < 0) & (k < words)).any())
                census["ragged_last"] |= bool(((lo + 16 > rb) & (k < words)).any())
                return np.where(inside, mem[aligned + k[:, None] * 16 + _J[None, :]], 0)

            carry63 = 0
            nxt = load(lanes)
            for base in range(0, words, LANES):
                v = nxt
                k = base + lanes
                if base + LANES < words:
                    nxt = load(k if defect == "prefetch_same_words" else k + LANES)
                lo = k * 16 - head
                lo0 = np.maximum(lo, 0)
                if not three:
                    cell_a = lo0 >> cell_shift
                    bnd = ((cell_a + 1) << cell_shift) - lo
                    if mode == LOW10:
                        b = np.where(((_J ^ head) & 1)[None, :] == 1, (v & 3) << 6, v >> 2)
                        if base > 0 and (lo[0] & 1):
                            census["low10_split_at_trip"] = True
                    elif mode == GRAY:
                        b = v
                    else:
                        sel = (1 if mode == UYVY else 0) ^ (head & 1)
                        b = np.where((_J & 1)[None, :] == sel, v, 0)
                    in_a = _J[None, :] < bnd[:, None]
                    sum_a, sum_b = (b * in_a).sum(axis=1), (b * ~in_a).sum(axis=1)
                else:
                    cell_a = lo0 // 48
                    bnd = (cell_a + 1) * 48 - lo
                    m = (lo + 48) % 3
                    e = (5 - m) % 3
                    ch = (m[:, None] + np.arange(3)[None, :]) % 3
                    wr = np.where(ch == 0, w_first, np.where(ch == 1, 150, w_last))
                    tail = np.where(e == 0, 0, np.where(e == 1, wr[:, 2] * v[:, 14], 0) + wr[:, 0] * v[:, 15])
                    acc = np.roll(tail, 1)                                   # __shfl_up(tail, 1) ...
                    acc[0] = carry63                                         # ... and lane 0 from the previous trip's lane 63
                    if defect != "carry_never":
                        carry63 = int(tail[62 if defect == "carry_lane62" else 63])
                    if base > 0:
                        census["e_at_trip"].add(int(e[0]))
                        census["boundary_mod3"].add(int(lo[0] % 3))
                    sum_a, sum_b = np.zeros(LANES, np.int64), np.zeros(LANES, np.int64)
                    for j in range(16):
                        acc = acc + wr[:, j % 3] * v[:, j]
                        ends = e == j % 3
                        luma = (acc + 128) >> 8
                        sum_a += np.where(ends & (j < bnd), luma, 0)
                        sum_b += np.where(ends & ~(j < bnd), luma, 0)
                        acc = np.where(ends, 0, acc)
                stores = (k < LANES) if defect == "guard_first_trip" else (k < words)
                add_a = stores & (sum_a != 0)
                add_b = stores & (sum_b != 0) & (cell_a + 1 < cols)
                census["zero_sum_skipped"] |= bool((stores & (sum_a == 0)).any())
                census["two_cells"] |= bool(add_b.any())
                census["last_cell_cut"] |= bool((stores & (bnd < 16) & (cell_a + 1 == cols)).any())
                assert (cell_a[add_a] < cols).all(), "an LDS add outside the strip's cells"
                np.add.at(cells, cell_a[add_a], sum_a[add_a])
                np.add.at(cells, cell_a[add_b] + 1, sum_b[add_b])
                if defect == "one_trip":
                    break
        out[strip] = (cells & 0xFFFF).astype(np.uint16)                      # t.now[at] = (uint16_t)s
    return out, census

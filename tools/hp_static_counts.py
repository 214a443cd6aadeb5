"""Static instruction counts and resources of the split-block kernels, from gfx950 listings (a compile, no GPU):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 --offload-device-only -S k_mbconv_hp.hip -o hp.s
    python tools/hp_static_counts.py before/hp.s after/hp.s [before/hp2.s after/hp2.s ...]  > profiles/..._static.txt

Per kernel of each before / after pair: instructions in all, VALU (v_* other than MFMAs), MFMAs, v_cndmask, vector compares, 64-bit
address arithmetic (v_lshl_add_u64, v_mad_u64_u32, v_mad_i64_i32), global / buffer loads, exec-mask saves (a waterfall loop around a
buffer load would show there) and the registers, static LDS (these kernels' LDS is dynamic: 0 here, sized by the launchers, which this
change does not touch), scratch and occupancy (waves per SIMD) the compiler reports at the end of each kernel."""
import re
import subprocess
import sys

ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32")
COLS = ("total", "valu", "mfma", "cndmask", "v_cmp", "addr64", "global_ld", "buffer_ld", "saveexec", "vgprs", "agprs", "sgprs", "lds", "scratch", "occ")


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: n for n in names}


def kernels(path):
    """mangled name -> dict of COLS"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            name, cur = m.group(1), dict.fromkeys(COLS, 0)
            continue
        if cur is None:
            continue
        s = line.strip()
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", s)
        if m:
            key = {"NumVgprs": "vgprs", "NumAgprs": "agprs", "TotalNumSgprs": "sgprs", "ScratchSize": "scratch", "Occupancy": "occ", "LDSByteSize": "lds"}[m.group(1)]
            cur[key] = int(m.group(2))
            if key == "occ":            # the last of the block
                out[name], cur = cur, None
            continue
        if not s or s[0] in ";." or s.endswith(":"):
            continue
        op = s.split()[0]
        if not re.match(r"^[a-z]", op):
            continue
        cur["total"] += 1
        if op.startswith("v_mfma"):
            cur["mfma"] += 1
        elif op.startswith("v_"):
            cur["valu"] += 1
        cur["cndmask"] += op.startswith("v_cndmask")
        cur["v_cmp"] += op.startswith("v_cmp")
        cur["addr64"] += op.startswith(ADDR64)
        cur["global_ld"] += op.startswith("global_load")
        cur["buffer_ld"] += op.startswith("buffer_load")
        cur["saveexec"] += "saveexec" in op
    return out


def main(paths):
    for before, after in zip(paths[0::2], paths[1::2]):
        kb, ka = kernels(before), kernels(after)
        names = demangle(sorted(set(kb) | set(ka)))
        print("%s -> %s" % (before, after))
        print("%-78s %-6s " % ("kernel", "") + " ".join("%9s" % c for c in COLS))
        for n in sorted(names, key=lambda n: names[n]):
            short = names[n].replace("void ", "").replace("(WzMbArgs)", "")
            for tag, k in (("before", kb.get(n)), ("after", ka.get(n))):
                if k is None:
                    print("%-78s %-6s (not in this listing)" % (short, tag))
                else:
                    print("%-78s %-6s " % (short if tag == "before" else "", tag) + " ".join("%9d" % k[c] for c in COLS))
            if kb.get(n) and ka.get(n):
                print("%-78s %-6s " % ("", "delta") + " ".join("%+9d" % (ka[n][c] - kb[n][c]) for c in COLS))
        print()


if __name__ == "__main__":
    main(sys.argv[1:])

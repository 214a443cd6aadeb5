"""Generates tests/golden/hp_halo_gather.json: SHA-256 of the output tensors of the split-operand blocks listed in
tests/hp_halo_gather.py, for the robust and the default program at batches 1, 2, 3 and 5.

Needs the GPU and the development library:   python tests/golden/make_hp_halo_gather_golden.py
Record on the commit whose tensors are to be kept, i.e. BEFORE a change of the blocks' loads that must not alter them.
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import hp_halo_gather as hg                                  # noqa: E402


def main():
    from watsor_amd.synth import synthetic_weights
    weights = synthetic_weights(hg.SEED)
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name in hg.PROGRAMS:
            prog = hg.program(name)
            e = hg.make_engine(name, tmp, weights)
            try:
                cases[name] = {str(n): hg.hashes_of_batch(e, prog, n) for n in hg.BATCHES}
            finally:
                e.close()
            print("%s: %d batches x %d blocks" % (name, len(cases[name]), len(cases[name]["1"])), flush=True)
    hg.write_golden(cases)
    print("wrote %s" % hg.PATH)


if __name__ == "__main__":
    main()

"""Generates tests/golden/network_launches.json: what every case of tests/launch_golden.py launches, as the libraries built from
the tree say it (kernel, workgroups, threads, LDS bytes per launch; graph nodes; the post-processing flags; the stage names; the
SHA-256 of the rows of fixed frames).

Needs the GPU and the measurement library (make -C watsor_amd/csrc stamps):   python tests/golden/make_network_launches_golden.py
One child process per environment, one after the other; the first child that fails ends the run and nothing is written.
Record on the commit whose launches are to be kept, i.e. BEFORE a change that must not alter them -- a hash that differs while the
launch list is equal means other ARGUMENTS (a K split, a workspace offset), which is a bug in the change, not a reason to record again.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import launch_golden as lg                                   # noqa: E402


def main():
    if not os.path.isfile(lg.STAMPS):
        sys.exit("%s is missing: make -C watsor_amd/csrc stamps" % lg.STAMPS)
    cases = {}
    with tempfile.TemporaryDirectory() as tmp:
        models_json = os.path.join(tmp, "models.json")
        with open(models_json, "w") as f:
            json.dump(lg.build_models(tmp), f)
        for env, (_, programs, _) in lg.ENVIRONMENTS.items():
            out_json = os.path.join(tmp, env + ".json")
            p = lg.run_child(env, programs, models_json, out_json, timeout=60 + 30 * len(programs))
            if p.returncode != 0:
                sys.exit("environment %s: the child ended with %d: nothing written\n%s" % (env, p.returncode, p.stderr[-3000:]))
            with open(out_json) as f:
                cases.update(json.load(f))
            print("%s: %d programs" % (env, len(programs)), flush=True)
    refused = [k for k, c in cases.items() for b in c["batches"].values() if not b["decode_fused"]]
    print("cases with a batch whose boxes the grouped reduce did not decode: %s" % (sorted(set(refused)) or "none"))
    lg.write_golden(cases)
    print("wrote %s (%d cases)" % (lg.PATH, len(cases)))


if __name__ == "__main__":
    main()

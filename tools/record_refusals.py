#!/usr/bin/env python3
"""Record what the library at hand answers to every argument set of tests/batch_refusal_cases.py: (return code, iyk_hip_last_error text)
per set, as JSON.  Run ONCE on the commit a refactor of the argument checks starts from (one MI355X), and commit the file as the refactor's
reference:   python tools/record_refusals.py [--out tests/golden/batch_refusals_parent.json]
One process.  A refused set returns before any launch; a legal set launches one to four jobs on zero-filled stores.  The sets with
debug = 1 run after a second iyk_hip_init under IYK_HIP_DEBUG=1.  The recording goes on only while every return code is IYK_OK,
IYK_ERR_INVALID, IYK_ERR_STATE or IYK_ERR_NOMEM: the first HIP error (or unknown code) ends it, and nothing is written."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "batch_refusals_parent.json"))
    out = ap.parse_args().out
    import batch_refusal_cases as cases
    from iyokan_amd import client, hip
    from iyokan_amd.params import params_128bit

    keys = client.keygen(params_128bit(), seed=1)
    got = {}
    for debug in (0, 1):
        os.environ["IYK_HIP_DEBUG"] = str(debug)   # read by iyk_hip_init
        hip.initialize(keys, device_ids=(0,))
        try:
            stores = cases.Stores(hip)
            for c in cases.CASES:
                if c["args"].get("debug", 0) != debug:
                    continue
                rc, text = stores.call(c)
                print(f"{c['id']}: {rc} {text}", flush=True)
                if rc not in (0, -1, -2, -4):
                    sys.exit(f"{c['id']}: return code {rc} ({text}): recording stopped, nothing written")
                got[c["id"]] = [rc, text]
            stores.free()   # synchronises the stream first: a fault of a legal set's launches shows here
        finally:
            hip.cleanup()
    with open(out, "w") as f:
        f.write('{"build_id": %s,\n "cases": {\n' % json.dumps(hip.build_id()))   # one set per line
        f.write(",\n".join("  %s: %s" % (json.dumps(i), json.dumps(got[i])) for i in sorted(got)))
        f.write("\n }}\n")
    print(f"{len(got)} sets recorded into {out}")


if __name__ == "__main__":
    main()

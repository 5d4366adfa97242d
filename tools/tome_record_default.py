#!/usr/bin/env python3
"""Record what the default path launches and computes: the entry-point sequence and the sha256 of the output bytes of the
workloads in tests/tome_default_path.py (the tiny golden forwards and the tiny denoising job), on an MI355X.

tests/golden/tome_default_launches.json was written by this tool run against the package as it stood on the commit before token
merging (the workloads use nothing newer); tests/test_tome_default_gpu.py holds every later tree to it.  `--package DIR` names
the directory that holds that `vdx/` (default: this tree).

    python tools/tome_record_default.py [--package DIR] --out tests/golden/tome_default_launches.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=ROOT)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.abspath(a.package))
    import torch
    import tome_default_path as D
    import vdx
    gpu = torch.device("cuda:0")
    rec = {"source_sha": vdx._lib.source_sha(), "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in D.WORKLOADS:
        out, seen = D.run(name, D.tiny_model(gpu), gpu)
        rec["workloads"][name] = {"launches": len(seen), "sha256": D.sha(out), "sequence": D.pack(seen)}
        print(name, len(seen), rec["workloads"][name]["sha256"])
    with open(a.out, "w") as f:
        f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

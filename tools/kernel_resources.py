#!/usr/bin/env python3
"""Condenses hipcc's -Rpass-analysis=kernel-resource-usage remarks (stderr of a build of csrc/ns_api.hip) into one line per
kernel: name, SGPRs, VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block, occupancy.  Sorted by name, so two
builds diff line by line.

    hipcc --offload-arch=gfx950 <the Makefile's flags> -Rpass-analysis=kernel-resource-usage ... 2> remarks.txt
    python tools/kernel_resources.py remarks.txt > profiles/correct/kernel_resources.txt
"""
import re
import subprocess
import sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occupancy")]


def main(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    names = sorted(rows)
    try:
        plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        plain = names
    for name, text in sorted(zip(names, plain), key=lambda p: p[1]):
        r = rows[name]
        print(re.sub(r"\(.*", "", text) + "  " + " ".join(f"{k}={r.get(k, '?')}" for _, k in FIELDS) + "  " + name)


if __name__ == "__main__":
    main(sys.argv[1])

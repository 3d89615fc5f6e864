"""Writes tests/golden/acosf_blocks.json: the restated glibc acosf of tests/cpp/fpfh_checker.c over all 2^32 float bit patterns,
compared with this platform's libm acosf (the count of differences is stored and must be 0), as 256 block checksums (the
format of atanf_blocks.json).  The GPU test evaluates the device's acosf against them.

    make && python tests/golden/gen_acosf_blocks.py
"""
import json
import os
import platform
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fpfh_checker as fc  # noqa: E402


def main():
    diffs, blocks = fc.acosf_exhaustive()
    if diffs:
        raise SystemExit(f"the restated acosf differs from libm on {diffs} inputs")
    out = {"what": "checksums of acosf over blocks of 2^24 consecutive float bit patterns (block b = bits b<<24 .. (b<<24)+2^24-1): "
                   "sum mod 2^64 of splitmix64((bits << 32) | result bits), NaN results counted as 0x7fc00000, from "
                   "tests/cpp/fpfh_checker.c:fpc_acosf_exhaustive",
           "libm": f"glibc {platform.libc_ver()[1]} acosf (plain FUNC, no IFUNC variant)",
           "differences_vs_libm": diffs, "blocks": blocks}
    with open(os.path.join(HERE, "acosf_blocks.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote acosf_blocks.json")


if __name__ == "__main__":
    main()

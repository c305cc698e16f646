"""Fixture of the frozen-plan test: tests/golden/many_plans.json, key -> [rc, workspace bytes, sha256 of the descriptor block] for
every plan tests/many_plan_cases.py enumerates.  It records what the host planners of the ragged calls WROTE, not what they should
write: the file is made once with the library of a commit whose plans are trusted, and tests/test_many_plans_frozen_cpu.py then holds
every later planner to the same bytes.

Run by hand, with that commit's library (no GPU, no Pillow):

    AA_INTERP_LIB=/path/to/that/build/libaa_interp.so python tests/golden/make_golden_many_plans.py

The committed file was made with the library built from commit 467775f ("Add resize_many_nearest"), the parent of the change that
moved the planners' shared checks into csrc/aa_many_host.h; the groups maps, ycbcr, err/maps and err/ycbcr were added with the library
built from commit b3940fe ("Add resize_many_ycbcr"), the parent of the change that gave the ragged kernels one device header
(csrc/aa_many_dev.h), and every older key came out of that library byte-equal to what was committed; the groups embed, back, merged,
back_bwd and their err/ groups were added with the library built from commit b51284d ("Add resize_many_back_merged"), the parent of
the change that gave the float ragged calls their shared headers (csrc/aa_float_many_dev.h, csrc/aa_float_many_host.h), again with
every older key byte-equal.  main() enumerates twice and asserts that both runs agree: the blocks are zero-initialised and the planners
memset their records, so the bytes do not depend on what the memory held."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "many_plans.json")


def digest():
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import many_plan_cases

    out = {}
    for key, rc, ws, block in many_plan_cases.plans():
        assert key not in out, key
        out[key] = [rc, ws, hashlib.sha256(block).hexdigest()]
    return out


def main() -> None:
    first, second = digest(), digest()
    assert first == second, "the planners' bytes differ between two runs"
    with open(OUT, "w") as f:
        json.dump(first, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{OUT}: {len(first)} plans, {sum(1 for v in first.values() if v[0] != 0)} of them errors")


if __name__ == "__main__":
    main()

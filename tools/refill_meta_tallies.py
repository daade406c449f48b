#!/usr/bin/env python3
"""Record the tally words tests/test_epa_refill_meta.py holds the refill tiers to: runs every case of that
file on the GPU with the library GJKEPA_LIB names and writes the selected route and seed tallies and the
park word of each case as JSON.  Run it on the build the counts are to come from (the commit before the
queue's metadata table, exported and built with tools/build_variant.sh SRCDIR=...), and commit the output
as tests/golden/epa_refill_meta_tallies.json.  The records are checked against the oracle on the way, so a
recording from a build that computes something else stops.
usage: GJKEPA_LIB=<libgjkepa_hip.so> python tools/refill_meta_tallies.py out.json"""
import inspect
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("collision-detect-gjk-epa_amd", "oracle", "tools", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import oracle  # noqa: E402
import test_epa_refill_meta as m  # noqa: E402


def main():
    oracle.load()
    out = {}

    def record(key, tally, park):
        assert key not in out, key
        out[key] = {"tally": [int(tally[i]) for i in m.TALLY_WORDS], "park": int(park)}

    m.expect_tallies = record
    fixtures = {"shapes": lambda: (m.shapes_pool(), oracle.gjkepa_batch(m.shapes_pool(), 2, 1.0)),
                "c5": lambda: m.c5_case(oracle)}
    made = {}
    for name, fn in inspect.getmembers(m, inspect.isfunction):
        if not name.startswith("test_"):
            continue
        marks = [mk for mk in getattr(fn, "pytestmark", []) if mk.name == "parametrize"]
        names = [mk.args[0].split(",") for mk in marks]
        for combo in itertools.product(*[mk.args[1] for mk in marks]):
            kw = {}
            for ns, val in zip(names, combo):
                kw.update(zip(ns, val if len(ns) > 1 else (val,)))
            for a in inspect.signature(fn).parameters:
                if a in fixtures:
                    if a not in made:
                        made[a] = fixtures[a]()
                    kw[a] = made[a]
            fn(**kw)
            print(name, {k: v for k, v in kw.items() if k not in fixtures}, "ok", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(f"{len(out)} cases -> {sys.argv[1]}")


if __name__ == "__main__":
    main()

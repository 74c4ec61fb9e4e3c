"""Writes tests/golden/hash_n_digest.json: for every input length 1..16 one fixed input vector
(hash_n_model.golden_inputs), its hash, and the sha256 of the oracle's trace rows and of its whole advice column
(oracle/trace.c, orc_hash_trace).  Provenance "oracle-trace": derived by the CPU oracle, KAT-anchored through the hash
(the output row), row ORDER unpinned by the reference."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hash_n_model as hn  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    orc = oracle_lib.load()
    res = {"provenance": "oracle-trace", "hashes": []}
    for length in hn.LENS:
        xs = hn.golden_inputs(length)
        t = hn.oracle_trace(orc, xs)
        res["hashes"].append({"len": length, "in": [str(x) for x in xs], "hash": str(orc.hash(xs)),
                              "rows": len(t["witness"]), "cells": len(t["cells"]),
                              "sha256_rows": hashlib.sha256(t["witness"].tobytes()).hexdigest(),
                              "sha256_cells": hashlib.sha256(t["cells"].tobytes()).hexdigest()})
    with open(os.path.join(ROOT, "tests", "golden", "hash_n_digest.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("wrote hash_n_digest.json:", len(res["hashes"]), "lengths")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""
Generates tests/golden/fri_vectors.json from the integer model of the FRI polynomial commitment (tests/fri_model.py; the
reference has no FRI, so the model is the only source):

    python tests/golden/gen_fri_golden.py

Per curve: one polynomial of 7 coefficients (fri_model.golden_poly, a BLAKE2b counter stream) under max_degree 8 (k = 3),
blowup 4, final 2 and 4 queries, opened at one point.  Stored: the parameters, the commitment, the value and the proof's bytes
(fri_model.proof_bytes), all hex.  The file pins the bytes: a change of the protocol shows up as a diff of this file.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import fri_model as M  # noqa: E402

SHAPE = {"k": 3, "b": 2, "f": 1, "queries": 4, "coefficients": 7}
POINT = 0x123456789ABCDEF0FEDCBA9876543210


def main():
    out = {}
    for seed, curve in enumerate(("BN254", "BLS12_381"), start=1):
        P = M.Params(curve, SHAPE["k"], SHAPE["b"], SHAPE["f"], SHAPE["queries"])
        poly = M.golden_poly(P.r, SHAPE["coefficients"], seed)
        root = M.commit(P, poly)[0]
        proof, values = M.prove(P, [poly], [(0, POINT)])
        assert M.verify(P, [root], [(0, POINT)], values, proof)
        out[curve] = dict(SHAPE, seed=seed, point=f"{POINT:x}", root=root.hex(), value=f"{values[0]:x}", proof=M.proof_bytes(proof).hex())
    path = os.path.join(HERE, "fri_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

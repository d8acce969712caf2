#!/usr/bin/env python3
"""
Generates tests/golden/merkle_vectors.json by RUNNING the reference's Merkle (python/zksnake/commitment/vector/merkle.py of a
zksnake source tree), loaded by path -- only that directory is imported, not the zksnake package, which needs its Rust extension:

    python tests/golden/gen_merkle_golden.py <zksnake source tree>

For n in SIZES the vector is leaf i = the byte i repeated i mod 5 times (tests/merkle_model.py golden_leaf: lengths 0..4, the
empty leaf among them).  Stored per n: the reference's commitment and, for every index, the reference's proof and whether the
reference's own verify accepts it (it does not where a node on the path had no right sibling: commit hashes such a node with itself,
open leaves the level out).  All values are hex.
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 16, 17)


def golden_leaf(i):
    return bytes([i & 0xFF]) * (i % 5)


def load_reference(tree):
    """the reference's commitment/vector directory as a package of its own"""
    pkg_dir = os.path.join(tree, "python", "zksnake", "commitment", "vector")
    spec = importlib.util.spec_from_file_location("ref_vector", os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["ref_vector"] = pkg
    spec.loader.exec_module(pkg)
    return pkg.Merkle


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    scheme = load_reference(sys.argv[1])()
    scheme.setup()
    out = {"alg": scheme.alg, "leaf_rule": "leaf i = bytes([i]) * (i % 5)", "trees": {}}
    for n in SIZES:
        vector = [golden_leaf(i) for i in range(n)]
        com = scheme.commit(vector)
        proofs = []
        for i in range(n):
            proof = scheme.open(vector, i)
            proofs.append({"proof": [p.hex() for p in proof], "verifies": bool(scheme.verify(com, proof, i, vector[i]))})
        out["trees"][str(n)] = {"root": com.hex(), "openings": proofs}
    path = os.path.join(HERE, "merkle_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

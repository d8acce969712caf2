"""The shape of a Merkle tree whatever its hash, written from the definition: every level with a lone node
hashed with itself, and an opening path with the node itself where it has no sibling.  merkle_model.py and poseidon_model.py bring
their hash as `parent(left, right)`."""


def levels(leaves, parent):
    """[level 0, level 1, .., [root]] from the leaf digests"""
    out = [list(leaves)]
    while len(out[-1]) > 1:
        cur = out[-1]
        out.append([parent(cur[i], cur[i + 1] if i + 1 < len(cur) else cur[i]) for i in range(0, len(cur), 2)])
    return out


def path(lv, index):
    """depth entries: the sibling at every level below the root, the node itself where there is none"""
    out = []
    for level in lv[:-1]:
        sib = index ^ 1
        out.append(level[sib] if sib < len(level) else level[index])
        index >>= 1
    return out

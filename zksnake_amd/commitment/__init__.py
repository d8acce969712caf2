"""Commitment schemes (the reference's `zksnake.commitment`): polynomial commitments (`commitment.polynomial`: KZG, IPA, multi-point
openings) and the vector commitment (`commitment.vector`: a BLAKE2b Merkle tree; section 4.12), on the GPU."""

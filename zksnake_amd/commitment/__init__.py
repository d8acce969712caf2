"""Commitment schemes (the reference's `zksnake.commitment`): polynomial commitments on the GPU.  The vector commitment (`Merkle`)
is not part of this package: its hot path is a blake2b kernel."""

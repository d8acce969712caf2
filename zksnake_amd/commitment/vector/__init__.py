"""Vector commitments (the reference's `zksnake.commitment.vector`): a BLAKE2b Merkle tree built on the GPU."""

from .base import VectorCommitmentScheme
from .merkle import Merkle, MerkleTree

__all__ = ["VectorCommitmentScheme", "Merkle", "MerkleTree"]

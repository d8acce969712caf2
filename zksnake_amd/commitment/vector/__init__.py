"""Vector commitments (the reference's `zksnake.commitment.vector`): a BLAKE2b Merkle tree and a Poseidon
Merkle tree over field elements, both built on the GPU."""

from .base import VectorCommitmentScheme
from .merkle import Merkle, MerkleTree
from .poseidon import PoseidonMerkle, PoseidonMerkleTree

__all__ = ["VectorCommitmentScheme", "Merkle", "MerkleTree", "PoseidonMerkle", "PoseidonMerkleTree"]

"""The reference's module path for the range proof; the code is ../range_proof.py."""

from ..range_proof import RangeProof, RangeProofObject

__all__ = ["RangeProof", "RangeProofObject"]

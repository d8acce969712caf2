"""The reference's import path (python/zksnake/subprotocol/bulletproofs/__init__.py): the inner-product argument of ../ipa.py and
the range proof of ../range_proof.py under the names code written against the reference imports."""

from ..ipa import InnerProductArgument, InnerProductProof
from ..range_proof import RangeProof, RangeProofObject

__all__ = ["InnerProductArgument", "InnerProductProof", "RangeProof", "RangeProofObject"]

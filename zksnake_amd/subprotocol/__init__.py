"""Interactive subprotocols (reference python/zksnake/subprotocol/): the sumcheck prover and verifier, the Bulletproofs
inner-product argument and range proof, and GKR for layered circuits."""

from .gkr import GKR, GkrPolynomial
from .ipa import InnerProductArgument, InnerProductProof
from .range_proof import RangeProof, RangeProofObject
from .sumcheck import ProductPolynomial, Sumcheck, SumcheckPolynomial

__all__ = ["GKR", "GkrPolynomial", "InnerProductArgument", "InnerProductProof", "ProductPolynomial", "RangeProof", "RangeProofObject",
           "Sumcheck", "SumcheckPolynomial"]

"""Interactive subprotocols (reference python/zksnake/subprotocol/): the sumcheck prover and verifier, the Bulletproofs
inner-product argument, and GKR for layered circuits."""

from .gkr import GKR, GkrPolynomial
from .ipa import InnerProductArgument, InnerProductProof
from .sumcheck import ProductPolynomial, Sumcheck, SumcheckPolynomial

__all__ = ["GKR", "GkrPolynomial", "InnerProductArgument", "InnerProductProof", "ProductPolynomial", "Sumcheck", "SumcheckPolynomial"]

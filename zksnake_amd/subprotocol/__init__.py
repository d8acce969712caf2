"""Interactive subprotocols (reference python/zksnake/subprotocol/): the sumcheck prover and verifier, and the Bulletproofs
inner-product argument."""

from .ipa import InnerProductArgument, InnerProductProof
from .sumcheck import ProductPolynomial, Sumcheck, SumcheckPolynomial

__all__ = ["InnerProductArgument", "InnerProductProof", "ProductPolynomial", "Sumcheck", "SumcheckPolynomial"]

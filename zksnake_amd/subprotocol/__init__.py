"""Interactive subprotocols (reference python/zksnake/subprotocol/): the sumcheck prover and verifier."""

from .sumcheck import ProductPolynomial, Sumcheck, SumcheckPolynomial

__all__ = ["ProductPolynomial", "Sumcheck", "SumcheckPolynomial"]

from .base import MultiOpeningQuery, PolynomialCommitmentScheme
from .fri import FRI, FriOracle, FriProof
from .ipa import IPA
from .kzg import KZG
from .mkzg import MultilinearKZG

__all__ = ["FRI", "FriOracle", "FriProof", "IPA", "KZG", "MultiOpeningQuery", "MultilinearKZG", "PolynomialCommitmentScheme"]

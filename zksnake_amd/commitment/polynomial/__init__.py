from .base import MultiOpeningQuery, PolynomialCommitmentScheme
from .ipa import IPA
from .kzg import KZG

__all__ = ["IPA", "KZG", "MultiOpeningQuery", "PolynomialCommitmentScheme"]

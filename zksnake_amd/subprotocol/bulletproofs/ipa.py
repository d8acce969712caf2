"""The reference's module path for the inner-product argument; the code is ../ipa.py."""

from ..ipa import InnerProductArgument, InnerProductProof

__all__ = ["InnerProductArgument", "InnerProductProof"]

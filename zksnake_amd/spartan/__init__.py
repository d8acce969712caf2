"""Spartan (https://eprint.iacr.org/2019/550, the NIZK variant) over the project's R1CS, sumcheck and multilinear KZG:
Spartan, SpartanProof."""

from .protocol import Spartan
from .serialization import SpartanProof

__all__ = ["Spartan", "SpartanProof"]

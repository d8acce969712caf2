"""Hash functions over the scalar field: Poseidon, on the host for one hash and on the GPU for many."""

from .poseidon import Poseidon

__all__ = ["Poseidon"]

"""What every vector commitment scheme of this package offers: the four methods of the reference's scheme, same argument meaning."""


class VectorCommitmentScheme:
    """setup() once, then commit(vector) -> commitment, open(vector, index) -> proof and
    verify(commitment, proof, index, element) -> bool.  `order` is None for schemes that are not over a field (Merkle)."""

    order = None

    def _missing(self, what):
        return NotImplementedError(f"{type(self).__name__} does not implement {what}()")

    def setup(self):
        raise self._missing("setup")

    def commit(self, vector):
        raise self._missing("commit")

    def open(self, vector, index):
        raise self._missing("open")

    def verify(self, commitment, proof, index, element):
        raise self._missing("verify")

"""
Byte layout of a Spartan proof (n = 32 / 48 bytes per compressed G1 point, scalars 32 bytes little-endian, h = s - 1):

  SpartanProof   s_x (1 byte) | s (1 byte) | C_w (G1) | outer rounds: s_x x 4 scalars | va | vb | vc
                 | inner rounds: s x 3 scalars | v_w | the opening: h points (G1)

`from_bytes` rejects (ValueError) a wrong length, a scalar that is not below r and a point that does not decode.
"""

from ..ecc import CurvePointSize, EllipticCurve

SCALAR_BYTES = 32


class SpartanProof:
    """commitment: C_w; outer: s_x rounds of 4 coefficients; evals: (va, vb, vc); inner: s rounds of 3 coefficients; v_w;
    opening: the h points of the multilinear KZG proof"""

    def __init__(self, commitment, outer, evals, inner, v_w, opening, curve="BN254"):
        self.commitment = commitment
        self.outer = [list(c) for c in outer]
        self.evals = tuple(evals)
        self.inner = [list(c) for c in inner]
        self.v_w = v_w
        self.opening = list(opening)
        self.curve = curve

    def __str__(self):
        return (f"C_w = {self.commitment}\nouter = {self.outer}\n(va, vb, vc) = {self.evals}\ninner = {self.inner}\n"
                f"v_w = {self.v_w}\nopening = {self.opening}")

    __repr__ = __str__

    @staticmethod
    def size(s_x, s, curve="BN254"):
        """bytes of a proof with s_x outer and s inner rounds"""
        return 2 + (s - 1 + 1) * CurvePointSize[curve].value + (4 * s_x + 3 + 3 * s + 1) * SCALAR_BYTES

    def to_bytes(self) -> bytes:
        s_x, s = len(self.outer), len(self.inner)
        scalars = lambda vals: b"".join(int(v).to_bytes(SCALAR_BYTES, "little") for v in vals)  # noqa: E731
        return (bytes([s_x, s]) + bytes(self.commitment.to_bytes()) + scalars(v for c in self.outer for v in c) + scalars(self.evals)
                + scalars(v for c in self.inner for v in c) + scalars([self.v_w]) + b"".join(bytes(q.to_bytes()) for q in self.opening))

    @classmethod
    def from_bytes(cls, data: bytes, crv="BN254"):
        data = bytes(data)
        E = EllipticCurve(crv)
        n, r = CurvePointSize[crv].value, E.order
        if len(data) < 2:
            raise ValueError("a Spartan proof starts with a header of 2 bytes")
        s_x, s = data[0], data[1]
        if s_x < 1 or s < 2 or len(data) != cls.size(s_x, s, crv):
            raise ValueError(f"a Spartan proof with s_x = {s_x}, s = {s} has {cls.size(s_x, max(s, 1), crv)} bytes, got {len(data)}")
        pos = [2]

        def point():
            pos[0] += n
            return E.curve.PointG1.from_bytes(data[pos[0] - n:pos[0]])       # ValueError when it does not decode

        def scalar():
            pos[0] += SCALAR_BYTES
            v = int.from_bytes(data[pos[0] - SCALAR_BYTES:pos[0]], "little")
            if v >= r:
                raise ValueError("a scalar of the proof is not below the group order")
            return v

        commitment = point()
        outer = [[scalar() for _ in range(4)] for _ in range(s_x)]
        evals = tuple(scalar() for _ in range(3))
        inner = [[scalar() for _ in range(3)] for _ in range(s)]
        v_w = scalar()
        opening = [point() for _ in range(s - 1)]
        return cls(commitment, outer, evals, inner, v_w, opening, crv)

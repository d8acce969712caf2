"""
The fixed G1 generators of an argument over Pedersen bases and everything that is derived from them, in one place: the
inner-product argument's (G, H) and the inner-product commitment's (G, h).  Nothing here is ever folded, so one MSM plan over
the concatenated bases serves every commitment, round and verification of the protocol that holds the set.
"""

import numpy as np

from .._algebra import PointArray
from ..transcript import FiatShamirTranscript


class GeneratorSet:
    """GeneratorSet(E, sizes): one part per entry of `sizes`, a PointArray of that many G1 points, or a single G1 point where
    the entry is None.  Derived lazily and dropped whenever a part is assigned: the concatenated bases (a PointArray, whose plan
    lives in HBM; slot 1 is a clone with a workspace and a stream of its own for the second MSM of a round), every part's
    compressed bytes, and the hasher of the default transcript after it has absorbed them."""

    def __init__(self, E, sizes):
        self.E = E
        self.sizes = sizes
        self.parts = [None] * len(sizes)
        self._bases = self._bytes = self._hasher = None

    def set(self, i, value):
        """part i = a PointArray or an iterable of sizes[i] points (a single point where sizes[i] is None)"""
        if self.sizes[i] is not None:
            value = PointArray.from_points(self.E.curve_id, 1, value, count=self.sizes[i], what="generators")
        elif not isinstance(value, self.E.curve.PointG1):
            raise TypeError("a single generator is a G1 point of the expected curve")
        self.parts[i] = value
        self._bytes = self._hasher = None
        self.release()

    def release(self):
        """free the MSM plans over the bases (they are rebuilt on the next use)"""
        if self._bases is not None:
            self._bases.release()
            self._bases = None

    def bases(self):
        """all parts back to back as one PointArray"""
        if self._bases is None:
            rows = [p.limbs if isinstance(p, PointArray) else p._limbs.reshape(1, -1) for p in self.parts]
            self._bases = PointArray(self.E.curve_id, 1, np.concatenate(rows))
        return self._bases

    def bytes(self):
        """per part, every point's compressed encoding back to back: what appending the points one by one adds to a transcript"""
        if self._bytes is None:
            self._bytes = [bytes(p.to_bytes()) for p in self.parts]
        return self._bytes

    def transcript(self, given, label, field):
        """the caller's transcript, or the default one FiatShamirTranscript(label, field), with every generator appended in part
        order.  The default transcript always starts with the same label and generators (64 MiB of them at 2^20 points), so its
        hasher is kept after the first use and copied."""
        fresh = given is None
        if fresh:
            given = FiatShamirTranscript(label, field)
            if self._hasher is not None:
                given.hasher = self._hasher.copy()
                return given
        for part in self.bytes():
            given.append(part)
        if fresh:
            self._hasher = given.hasher.copy()
        return given

    def msm(self, vec, count, timings=None):
        """<vec[:count], bases[:count]> for a device vector"""
        return self.bases().msm(vec, count, timings=timings)

    def msm_lr(self, scal_l, scal_r, count, profile=False):
        """(L, R, msm_ms): the two MSMs of a round over the first `count` bases, in flight together, each on its plan's stream --
        or, with profile, one after the other so that each run's milliseconds can be read (their sum is msm_ms, else 0)"""
        bases = self.bases()
        if profile:
            ms = []
            return bases.msm(scal_l, count, timings=ms), bases.msm(scal_r, count, timings=ms), sum(ms)
        left = bases.msm_enqueue(scal_l, count)
        right = bases.msm_enqueue(scal_r, count, slot=1, concurrent=True)
        return bases.msm_finish(left), bases.msm_finish(right), 0.0


def round_profile(k, t0, t1, t2, t3, msm_ms):
    """the profile record of round k from its four perf_counter readings: kernel, MSMs, host algebra"""
    return {"round": k, "kernel_ms": (t1 - t0) * 1e3, "msm_wall_ms": (t2 - t1) * 1e3, "msm_ms": msm_ms, "host_ms": (t3 - t2) * 1e3}

"""Beam profiles as convolution taps: the share of a beam's power that falls into each (x, y) column of voxels about the
beam's centre, which is the centre of a column.  Convolving the tally of a pencil beam with these taps
(PhotonTracer.beam_response, Context.tally_convolve) gives the response of a laterally uniform medium to the whole beam.

Host only: NumPy and math.erf; nothing here loads the library.
"""
import math

import numpy as np

MAX_TAPS_2D = 63      # lt_tally_convolve / lt_tally_convolve_at: taps per axis
MAX_TAPS_SEP = 255    # lt_tally_convolve_sep


def _voxel_xy(voxel_xy):
    v = tuple(float(d) for d in (voxel_xy if np.ndim(voxel_xy) else (voxel_xy, voxel_xy)))[:2]
    if len(v) != 2 or not all(d > 0 and math.isfinite(d) for d in v):
        raise ValueError("voxel_xy = %r: two positive sizes (dx, dy)" % (voxel_xy,))
    return v


class GaussianProfile:
    """A Gaussian beam of 1/e^2 radius ``radius`` (irradiance ~ exp(-2 r^2 / radius^2)) carrying ``power``.  It is the product
    of a profile in x and one in y, so the taps are a pair for the separable convolution; they reach ``extent`` radii from the
    centre, rounded up to whole columns (2.5 radii leave about 1e-6 of the power outside: cut_off())."""

    def __init__(self, radius, power=1.0, extent=2.5):
        self.radius, self.power, self.extent = float(radius), float(power), float(extent)
        if not (self.radius > 0 and math.isfinite(self.radius)) or not (self.power >= 0 and math.isfinite(self.power)) or not self.extent > 0:
            raise ValueError("GaussianProfile: radius > 0, power >= 0 and extent > 0, all finite")
        self._voxel = None

    def half_width(self, d):
        return int(math.ceil(self.extent * self.radius / d))

    def _axis(self, d):
        h = self.half_width(d)
        if 2 * h + 1 > MAX_TAPS_SEP:
            raise ValueError("GaussianProfile(radius=%g, extent=%g) on voxels of %g needs %d taps along an axis, the library takes %d: "
                             "voxels of %g or more would fit" % (self.radius, self.extent, d, 2 * h + 1, MAX_TAPS_SEP,
                                                                 self.extent * self.radius / (MAX_TAPS_SEP // 2)))
        s = math.sqrt(2.0) / self.radius
        return np.array([0.5 * (math.erf(s * ((k + 0.5) * d)) - math.erf(s * ((k - 0.5) * d))) for k in range(-h, h + 1)])

    def taps(self, voxel_xy):
        """(taps_x, taps_y): tap k of an axis is the exact share of the power between the edges a, b of the column k - h columns
        from the centre, 0.5 (erf(sqrt2 b / R) - erf(sqrt2 a / R)); 2 ceil(extent R / d) + 1 taps; ``power`` is in taps_x."""
        dx, dy = _voxel_xy(voxel_xy)
        tx, ty = self._axis(dx), self._axis(dy)
        self._voxel = (dx, dy)
        return self.power * tx, ty

    def cut_off(self, voxel_xy=None):
        """The share of the power outside the taps, for ``voxel_xy`` or the voxels of the last taps() call."""
        v = _voxel_xy(voxel_xy) if voxel_xy is not None else self._voxel
        if v is None:
            raise ValueError("cut_off(): give voxel_xy, or call taps(voxel_xy) first")
        s = math.sqrt(2.0) / self.radius
        inside = [math.erf(s * ((self.half_width(d) + 0.5) * d)) for d in v]
        return 1.0 - inside[0] * inside[1]


class FlatTopProfile:
    """A beam of uniform irradiance inside ``radius`` carrying ``power``.  Every column is cut into subsamples x subsamples
    cells; a tap is the column's share of the cells whose midpoint lies inside the disc."""

    def __init__(self, radius, power=1.0, subsamples=16):
        self.radius, self.power, self.subsamples = float(radius), float(power), int(subsamples)
        if not (self.radius > 0 and math.isfinite(self.radius)) or not (self.power >= 0 and math.isfinite(self.power)) or self.subsamples < 1:
            raise ValueError("FlatTopProfile: radius > 0, power >= 0 (finite) and subsamples >= 1")

    def taps(self, voxel_xy):
        """float64 [kh, kw], odd counts: power * (cell midpoints of the column inside the disc) / (cell midpoints inside the
        disc).  The counts are integers taken at midpoints that mirror exactly, so the taps are equal under both flips bit for
        bit; a disc that holds no midpoint at all (far smaller than a cell) is the single tap ``power``."""
        dx, dy = _voxel_xy(voxel_xy)
        s = self.subsamples
        hx, hy = int(math.ceil(self.radius / dx)), int(math.ceil(self.radius / dy))
        if 2 * max(hx, hy) + 1 > MAX_TAPS_2D:
            raise ValueError("FlatTopProfile(radius=%g) on voxels of (%g, %g) needs %d taps along an axis, the library takes %d: voxels "
                             "of %g or more would fit" % (self.radius, dx, dy, 2 * max(hx, hy) + 1, MAX_TAPS_2D,
                                                          self.radius / (MAX_TAPS_2D // 2)))
        # midpoint m of column k lies at (2 s k + 2 m + 1 - s) * d / (2 s): odd or even integers u that mirror exactly
        ux = (2 * s * np.arange(-hx, hx + 1)[:, None] + 2 * np.arange(s)[None, :] + 1 - s).astype(np.float64) * dx
        uy = (2 * s * np.arange(-hy, hy + 1)[:, None] + 2 * np.arange(s)[None, :] + 1 - s).astype(np.float64) * dy
        inside = (uy * uy)[:, None, :, None] + (ux * ux)[None, :, None, :] <= (2.0 * s * self.radius) ** 2      # [ky, kx, my, mx]
        count = inside.sum(axis=(2, 3))
        total = int(count.sum())
        if total == 0:
            return np.array([[self.power]])
        ys, xs = np.flatnonzero(count.sum(axis=1)), np.flatnonzero(count.sum(axis=0))
        count = count[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]      # the counts mirror: what is cut off is cut off on both sides
        return self.power * (count.astype(np.float64) / float(total))

    def cut_off(self, voxel_xy=None):
        return 0.0

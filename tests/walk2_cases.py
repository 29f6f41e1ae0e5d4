"""The inputs of the two-term strip walk's tests, built on the host alone: tests/test_gpu_walk2_forms.py runs them through cheby!
with the terms in pairs, tests/test_walk2_step_ref.py (no GPU) shows on the same lattices that the row-wise bound of
tests/walk2_step_ref.py catches every mutation of a pair launch.

A lattice is periodic (synth.hermitian_offsets_csr: row i couples to i +- d mod N): NN near distances of at most 16 rows, K far
distances g, 2 g .. K g, with or without a diagonal, complex couplings or real ones (the library then streams its real copy of
the values).  The rows within K g of either end wrap around and fall out of the uniform run, so in 64-row blocks, S = g / 64:

    the run                      [R0, R1) = [ceil(K g / 64), min(N // 64, (N - K g) // 64))
    the one-term walk            [R0 + K S, R1)                     (walk_info: first_block, end_block)
    the two-term region          [R0 + 2 K S, R1 - K S)             (walk2_info), everything else an edge block

which Lattice.plan() states and the GPU test compares with what the library planned.  BUILDERS: one lattice per (NN, K, diagonal,
real), g = 64 and N = 64 (6 K + 16) -- the region is K + 16 strip steps, at least the 2 K + 4 of a run-in and a few steps more; the
largest near distance varies over the shapes (DMAX; 1 and 16 are there).  GEOMETRY: what the chunks, the last block and the strip
step can be, on a few shapes, each case named for what it reaches.  cuts(): values of walk_waves, named likewise.

State vectors: cases.scaled_vector (nonzero everywhere: every row has a magnitude).  Delta = 26, E_min = -12: the spectrum
(Gershgorin: within +-11) lies inside, beta = 1 and the phase exp(-i dt) are not trivial."""
import dataclasses
import functools
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cheby_term_cases as cases  # noqa: E402
import walk2_step_ref as W2  # noqa: E402

KNOBS = dict(cases.KEEP, colblock=0, hrb_walk=1, walk_pair=1, walk_min_blocks=8, acc_defer=1)
DELTA, E_MIN, DT = 26.0, -12.0, 0.5

# largest near distance of the shape (NN, K): DMAX[NN - 1][K - 1]
DMAX = ((1, 16, 5, 9), (2, 16, 7, 12), (3, 16, 8, 13), (4, 16, 10, 6))


def near_distances(nn, dmax, seed):
    assert 1 <= nn <= min(4, dmax) and dmax <= 16
    rng = np.random.default_rng(seed)
    return tuple(sorted(int(d) for d in rng.choice(np.arange(1, dmax), nn - 1, replace=False))) + (dmax,)


@dataclasses.dataclass(frozen=True)
class Lattice:
    name: str
    nn: int
    K: int
    diag: int
    real: bool
    g: int
    n: int
    near: tuple

    @property
    def dmax(self):
        return self.near[-1]

    @property
    def shape(self):
        return (self.nn, self.K, self.diag)

    @property
    def offsets(self):
        return self.near + tuple(self.g * m for m in range(1, self.K + 1))

    @property
    def seed(self):
        return zlib.crc32(self.name.encode())

    def plan(self):
        """one-term walk [first_block, end_block), two-term region [first_block, end_block), edge blocks of the two-term plan"""
        S = self.g // 64
        R0, R1 = -(-self.K * self.g // 64), min(self.n // 64, (self.n - self.K * self.g) // 64)
        one = (R0 + self.K * S, R1)
        two = (R0 + 2 * self.K * S, R1 - self.K * S)
        return dict(one=one, two=two, edge2=-(-self.n // 64) - (two[1] - two[0]), strip_steps=-(-(two[1] - two[0]) * 64 // self.g))

    def geometry(self):
        two = self.plan()["two"]
        return W2.Geometry(self.n, self.g, self.K, self.dmax, 64 * two[0], 64 * two[1])

    def chunks(self):
        """column chunks per strip step: ceil(g / W)"""
        return -(-self.g // (64 - 2 * self.dmax))

    def matrix(self):
        A = cases.lattice(self.n, self.offsets, diag=bool(self.diag), real=self.real)
        assert np.all(np.diff(A.indptr) == 2 * (self.nn + self.K) + self.diag)
        return A

    def psi(self, k=0):
        return cases.scaled_vector(self.n, self.seed + k)


def _lattice(name, nn, K, diag, real, g, n, dmax):
    lat = Lattice(name, nn, K, diag, real, g, n, near_distances(nn, dmax, zlib.crc32(name.encode())))
    p = lat.plan()
    assert g % 64 == 0 and 2 * max(lat.offsets) < n
    assert p["one"][1] - p["one"][0] >= KNOBS["walk_min_blocks"], name
    assert p["strip_steps"] >= 2 * K + 4 and (p["two"][1] - p["two"][0]) >= 8 * (g // 64), name       # (the plan's own floor: 8 S)
    return lat


def shape_name(nn, K, diag, real):
    return f"nn{nn}k{K}d{diag}-{'real' if real else 'complex'}"


BUILDERS = {}
for _nn in (1, 2, 3, 4):
    for _K in (1, 2, 3, 4):
        for _diag in (0, 1):
            for _real in (False, True):
                BUILDERS[shape_name(_nn, _K, _diag, _real)] = functools.partial(
                    _lattice, shape_name(_nn, _K, _diag, _real), _nn, _K, _diag, _real, 64, 64 * (6 * _K + 16), DMAX[_nn - 1][_K - 1])
BUILDER_NAMES = list(BUILDERS)
assert len(BUILDERS) == 64 and max(64 * (6 * K + 16) for K in (1, 2, 3, 4)) == 2560

# the shapes of the geometry cases and of test_every_pair_form
SHAPES = {"nn4k4d0-complex": (4, 4, 0, False), "nn2k2d1-real": (2, 2, 1, True), "nn1k1d1-complex": (1, 1, 1, False),
          "nn3k1d0-complex": (3, 1, 0, False)}
PAIR_FORM_LATTICES = ("nn4k4d0-complex", "nn2k2d1-real")


def _rows(K, g, extra=0):
    """the smallest lattice of strip step g whose two-term region has 2 K + 4 strip steps, the plan's floor of 8, and a count of
    steps that some segment length does not divide (12 has none: 13): (5 K + steps) g rows"""
    steps = max(2 * K + 4, 8)
    while all(steps % -(-steps // t) == 0 for t in range(2, steps)):
        steps += 1
    return (5 * K + steps) * g + extra


# name -> (g, dmax, rows beyond _rows, the shapes that can have it: dmax >= NN, and at most 2560 rows unless g = 1024)
GEOMETRY = {
    "W_divides_g-dmax16-g64": (64, 16, 0, tuple(SHAPES)),                       # W = 32: two chunks, both fully owned
    "W_divides_g-dmax8-g192": (192, 8, 0, ("nn1k1d1-complex", "nn3k1d0-complex")),       # W = 48: four chunks
    "last_chunk_partly_owned-dmax4-g64": (64, 4, 0, tuple(SHAPES)),             # W = 56: the second chunk owns 8 rows
    "dmax1-W62-g64": (64, 1, 0, ("nn1k1d1-complex",)),
    "N_no_multiple_of_64-g64": (64, 5, 37, tuple(SHAPES)),                      # a partly filled last row block
    "N_no_multiple_of_g-g128": (128, 6, 64, ("nn2k2d1-real", "nn1k1d1-complex", "nn3k1d0-complex")),
    "g1024-dmax4": (1024, 4, 0, tuple(SHAPES)),                                 # the headline's strip step: 19 chunks of 56
}
GEOMETRY_CASES = [(geo, shape) for geo, spec in GEOMETRY.items() for shape in spec[3]]


def geometry_lattice(geo, shape):
    g, dmax, extra, shapes = GEOMETRY[geo]
    assert shape in shapes
    nn, K, diag, real = SHAPES[shape]
    n = (1 << 15) if g == 1024 else _rows(K, g, extra)
    assert n <= 2560 or (g == 1024 and n <= 1 << 15)
    return _lattice(f"{geo}/{shape}", nn, K, diag, real, g, n, dmax)


def geometry_property(geo, lat):
    """does the lattice have the property its case is named for?"""
    W = 64 - 2 * lat.dmax
    return {"W_divides_g-dmax16-g64": lat.g % W == 0 and lat.dmax == 16, "W_divides_g-dmax8-g192": lat.g % W == 0 and lat.dmax == 8,
            "last_chunk_partly_owned-dmax4-g64": lat.g % W != 0, "dmax1-W62-g64": W == 62, "N_no_multiple_of_64-g64": lat.n % 64 != 0,
            "N_no_multiple_of_g-g128": lat.n % lat.g != 0 and lat.n % 64 == 0, "g1024-dmax4": lat.g == 1024}[geo]


# ---- cuts -------------------------------------------------------------------------------------------------------------------
CUTS = ("one_step_per_wavefront", "whole_run_per_wavefront", "short_last_segment", "idle_wavefronts")


def cut_of(walk_waves, strip_steps, chunks):
    """(steps_per_wavefront, segments) of a two-term launch with this walk_waves (csrc/walk_geometry.cpp: walk2_cut)"""
    target = max(1, walk_waves // chunks)
    L = -(-strip_steps // target)
    return L, -(-strip_steps // L)


def cut_property(cut, info, strip_steps):
    L, nseg, chunks = info["steps_per_wavefront"], info["segments"], info["chunks_per_strip_step"]
    return {"one_step_per_wavefront": L == 1 and nseg == strip_steps,
            "whole_run_per_wavefront": L == strip_steps and nseg == 1,
            "short_last_segment": nseg >= 2 and strip_steps % L != 0 and (nseg - 1) * L < strip_steps < nseg * L,
            "idle_wavefronts": (nseg * chunks) % 4 != 0}[cut]


def cuts(lat):
    """name -> walk_waves for the cuts this lattice can have (idle wavefronts: not when every count of segments x chunks is a
    multiple of the workgroup's four wavefronts)"""
    J, S2 = lat.plan()["strip_steps"], lat.chunks()
    out = {"one_step_per_wavefront": J * S2, "whole_run_per_wavefront": 1}
    for cut in ("short_last_segment", "idle_wavefronts"):
        for target in range(2, J + 1):
            L, nseg = cut_of(target * S2, J, S2)
            if cut_property(cut, dict(steps_per_wavefront=L, segments=nseg, chunks_per_strip_step=S2), J) and L > 1:
                out[cut] = target * S2
                break
    return out

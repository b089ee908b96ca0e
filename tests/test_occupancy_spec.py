"""The tiers' occupancy bitmap, ray skip and classifier (csrc/tier.hpp) against a plain float64 specification.

tests/test_tiered.py, test_render_maps.py, test_tier_audit.py and test_posed_query.py see the bitmap only where a fixture's rays or
points happen to land.  Here every step that decides what is NOT computed is held to a numpy float64 restatement of the same step,
fed with the step's inputs AS THE BUFFER HOLDS THEM (hip.occupancy_view): csdf for the refinement, fsdf and cell_lip for the
selection, sel_bar and cell_stretch for the marking, bits for the distances, dist for the ray skip -- each kernel is judged on its own
-- plus one end-to-end property against the float64 oracle that uses none of the buffer's intermediates.

A comparison the kernel makes in fp32 and the restatement in float64 cannot be demanded bit for bit AT the threshold: an element
whose decision quantity lies within the stated shell of its threshold is UNDECIDED and may go either way, everything else agrees
with no exception, and the share of undecided elements is capped (printed by every test: ``occupancy_spec | ...``).

  refinement / selection   shell: a relative 1e-5 of the threshold band_n            cap 0.1 % of the refined cells / selected points
  marking                  shell: 1e-4 voxels around the kernel's own radius          cap 0.1 % of the marked voxels
  distances                none: exact
  ray skip                 soundness and tightness without exception; rays with an end within 1e-3 voxels of a box face are left
                           out of the tightness rule, at most 1 % of the rays
  classifier               a sample is undecided if moving it 1e-4 voxels along an axis changes its (marked, dist); rays with one
                           are left out, at most 1 % of the rays

The restatements themselves are tested first, without a GPU, against something more naive (test_spec_*): the L1 transform against
an O(n^2) brute force, the ball marker against a k-d tree, the segment test against dense sampling, the classifier on hand-written
rays.
"""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO, golden, get_model
from oracle import arah_oracle as O
from test_pointwise_f64 import ENGINES, chunked, hip_frame

gpu = pytest.mark.gpu

F64 = np.float64
SQ3H = float(np.float32(0.8660254))          # the kernels' half diagonal of a unit cube, as fp32 holds it
CANARY = 0xA5
SHELL_REL = 1e-5                             # refinement / selection: relative shell of the threshold
MARK_EPS = 1e-4                              # marking: voxels around the radius
CAP = 1e-3                                   # undecided share of refinement, selection, marking
RAY_FACE_EPS, RAY_CAP = 1e-3, 1e-2           # ray skip: ends near a box face, their share
CLS_EPS, CLS_CAP = 1e-4, 1e-2                # classifier: the undecided samples' move, the share of rays left out
SUB = 16                                     # segment samples per voxel
DEEP = 1e-2                                  # "deep inside a voxel" of the face-neighbour rule (test_ray_skip...)
TS_NONE, TS_PHASE1, TS_PENDING, TS_PHASE2 = 0, 1, 2, 3


@pytest.fixture(scope="module", autouse=True)
def _at_most_16_threads():
    prev = torch.get_num_threads()
    torch.set_num_threads(min(16, prev))
    yield
    torch.set_num_threads(prev)


def report(what, tag, undecided, of, cap):
    share = undecided / max(of, 1)
    print("occupancy_spec | %-12s %-24s undecided %7d of %9d = %.5f %% (cap %.3g %%)" % (what, tag, undecided, of, 100 * share, 100 * cap))
    assert undecided <= cap * of, (what, tag, undecided, of)


# =====================================================================================================================
# the layout (CPU)
# =====================================================================================================================
def _tier_source():
    src = open(os.path.join(REPO, "arah_release_amd", "csrc", "tier.hpp")).read()
    const = {}
    for decl in re.findall(r"^constexpr (?:int|float) ([^;]+);", src, re.M):
        for name, val in re.findall(r"(k\w+) = ([^,;]+)", decl):
            const[name] = val.strip()
    return src, const


def test_occupancy_view_follows_the_kernel_source():
    """hip.occupancy_view decodes the occupancy buffer: its field order is carve_occ's, its constants are tier.hpp's, its alignment
    Carver::take's, and OccInfo is the 16 words the view says."""
    from arah_release_amd import hip
    src, const = _tier_source()
    val = lambda k: float(const[k].rstrip("f")) if "." in const[k] else int(eval(const[k], {}, {}))
    assert (val("kOccNc"), val("kOccF"), val("kOccMaxCells"), val("kOccMaxVox")) == (hip.OCC_NC, hip.OCC_F, hip.OCC_MAX_CELLS, hip.OCC_MAX_VOX)
    assert (val("kOccL"), val("kTierBand")) == (hip.OCC_L, hip.TIER_BAND)
    assert const["kOccF3"] == "kOccF * kOccF * kOccF" and const["kOccMaxFine"] == "kOccMaxCells * kOccF3"
    assert hip.OCC_MAX_FINE == hip.OCC_MAX_CELLS * hip.OCC_F ** 3
    body = re.search(r"struct OccInfo \{(.*?)\};", src, re.S).group(1)
    fields = [(t, n.strip()) for t, decl in re.findall(r"^\s*(float|int) ([^;]+);", body, re.M) for n in decl.split(",")]
    assert fields == [("float", "origin[3]"), ("float", "v"), ("float", "inv_v"), ("int", "dims[3]"), ("int", "n_vox"), ("int", "valid"),
                      ("int", "n_cells"), ("int", "n_fine"), ("int", "n_sel"), ("int", "overflow"), ("float", "band_m"), ("float", "lip_pose")]
    assert hip.OCC_INFO_WORDS == 16 == sum(3 if "[3]" in n else 1 for _, n in fields)
    host = open(os.path.join(REPO, "arah_release_amd", "csrc", "arah_hip.hip")).read()
    carve = re.search(r"static OccBuf carve_occ\(void\* base\) \{(.*?)\n\}", host, re.S).group(1)
    takes = re.findall(r"o\.(\w+) = c\.take<(\w+)>\(([^;]+)\);", carve)
    sym = {"kOccNc": hip.OCC_NC, "kOccMaxVox": hip.OCC_MAX_VOX, "kOccMaxCells": hip.OCC_MAX_CELLS, "kOccMaxFine": hip.OCC_MAX_FINE}
    ctype = {"OccInfo": (torch.int32, 16), "unsigned": (torch.int32, 1), "uint8_t": (torch.uint8, 1), "float": (torch.float32, 1), "int": (torch.int32, 1)}
    assert [t[0] for t in takes] == [f[0] for f in hip.OCC_FIELDS]
    for (name, ct, expr), (fname, dt, shape) in zip(takes, hip.OCC_FIELDS):
        count = int(eval(expr.replace("(size_t)", ""), {}, sym))
        assert ctype[ct][0] == dt and count * ctype[ct][1] == int(np.prod(shape)), name
    assert "o.bytes = align_up(c.off, 256);" in carve
    take = re.search(r"struct Carver \{(.*?)\n\};", host, re.S).group(1)
    assert "off = align_up(off, 256);" in take and hip.OCC_ALIGN == 256
    layout, total = hip.occupancy_layout()
    end = 0
    for name, off, nbytes, dt, shape in layout:
        assert off % 256 == 0 and 0 <= off - end < 256, name
        end = off + nbytes
    assert total == (end + 255) // 256 * 256
    buf = torch.zeros(total, dtype=torch.uint8)
    view = hip.occupancy_view(buf)
    assert list(view) == [f[0] for f in hip.OCC_FIELDS]
    view["sel_of"][-1] = -1                      # zero-copy: a write through the view lands in the buffer's last array
    assert int(buf[layout[-1][1] + layout[-1][2] - 4:layout[-1][1] + layout[-1][2]].view(torch.int32)[0]) == -1
    with pytest.raises(ValueError):
        hip.occupancy_view(buf[:-1])


# =====================================================================================================================
# the restatement (numpy, float64)
# =====================================================================================================================
def spec_lattice(nc, L):
    """k_occ_lattice_pts: point i = (ix * nc + iy) * nc + iz sits at -L + 2 L / (nc - 1) * (ix, iy, iz)."""
    ax = -L + (2.0 * L / (nc - 1)) * np.arange(nc, dtype=F64)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


def spec_refine(csdf, nc, L):
    """k_occ_cells on the coarse values: per cell [cx, cy, cz] the decision quantity q = min(corners) - lip * half diagonal (the cell
    is refined when q <= band_n), its constant lip = max(1.5, 1.25 x steepest slope along the twelve edges) and whether it lies on
    the lattice's boundary."""
    m = nc - 1
    v = np.asarray(csdf, F64).reshape(nc, nc, nc)
    step = 2.0 * L / m
    sh = [(slice(i, i + m), slice(j, j + m), slice(k, k + m)) for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    mn = np.min([v[s] for s in sh], axis=0)
    sl = np.zeros((m, m, m))
    for a in (0, 1):
        for b in (0, 1):
            sl = np.maximum(sl, np.abs(v[1:, a:a + m, b:b + m] - v[:-1, a:a + m, b:b + m]))
            sl = np.maximum(sl, np.abs(v[a:a + m, 1:, b:b + m] - v[a:a + m, :-1, b:b + m]))
            sl = np.maximum(sl, np.abs(v[a:a + m, b:b + m, 1:] - v[a:a + m, b:b + m, :-1]))
    lip = np.maximum(1.5, 1.25 * sl / step)
    idx = np.arange(m)
    e1 = (idx == 0) | (idx == m - 1)
    edge = e1[:, None, None] | e1[None, :, None] | e1[None, None, :]
    return mn - lip * (step * SQ3H), lip, edge


_OFF27 = np.stack([np.arange(27) // 9, (np.arange(27) // 3) % 3, np.arange(27) % 3], -1).astype(F64)   # fine point j -> (a, b, d)
_D27 = np.sqrt(((_OFF27[:, None] - _OFF27[None]) ** 2).sum(-1))                                       # lattice distance of two


def spec_fine_lattice(cells, nc, L):
    """The 3 x 3 x 3 cell-centred sub-lattice of the coarse cells (n, 3) -> (n, 27, 3)."""
    step = 2.0 * L / (nc - 1)
    return -L + step * np.asarray(cells, F64)[:, None, :] + (step / 3.0) * (_OFF27[None] + 0.5)


def spec_pair_max(val, ok, spacing):
    """max over the pairs (a, b) of a cell's fine points with ok[a] and ok[b] of |val[a] - val[b]| / (spacing x lattice distance);
    val (n, 27, k), ok (n, 27) -> (n,), 0 without a pair."""
    out = np.zeros(val.shape[0])
    den = np.where(_D27 > 0, _D27, np.inf) * spacing
    for c in range(0, val.shape[0], 512):
        d = np.sqrt(((val[c:c + 512, :, None, :] - val[c:c + 512, None, :, :]) ** 2).sum(-1)) / den
        d = np.where(ok[c:c + 512, :, None] & ok[c:c + 512, None, :], d, 0.0)
        out[c:c + 512] = d.max((1, 2))
    return out


def spec_cell_lip(coarse_lip, edge, fsdf27, nc, L):
    """k_occ_cells + k_occ_cell_slope: max(coarse constant, 1.25 x steepest slope between the cell's 27 fine values) for interior cells,
    minus the coarse constant for cells on the lattice's boundary."""
    fs = 2.0 * L / (nc - 1) / 3.0
    fine = spec_pair_max(np.asarray(fsdf27, F64)[:, :, None], np.ones(fsdf27.shape, bool), fs)
    return np.where(edge, -coarse_lip, np.maximum(coarse_lip, 1.25 * fine))


def spec_select_quantity(fsdf, cell_lip, nc, L):
    """k_occ_select: a fine point is selected unless fsdf - |cell_lip| x half fine diagonal > band_n; -> that quantity per fine point."""
    half = 2.0 * L / (nc - 1) / 3.0 * SQ3H
    return np.asarray(fsdf, F64) - np.abs(np.repeat(np.asarray(cell_lip, F64), 27)) * half


def spec_unnormalize(x, cmin, cmax, center):
    """RFU:47-51 in float64; also the largest magnitude among the terms of the sum (the scale of its fp32 rounding)."""
    rng = cmax - cmin
    a = (np.asarray(x, F64) / 2.0 + 0.5) * 1.1 * rng
    out = a + cmin - rng * 0.05 + center
    mag = np.maximum.reduce([np.abs(a), np.abs(out), np.full_like(a, abs(cmin)), np.broadcast_to(np.abs(center), a.shape)])
    return out, mag


def spec_mark(p, rad, dims, eps):
    """k_occ_mark: p (n, 3) images in voxel units relative to the voxel CENTRES (voxel k sits at k), rad (n,) radii in voxels,
    dims (dx, dy, dz).  -> (must, may), bool [dz, dy, dx]: voxels nearer than rad - eps to some image, voxels within rad + eps."""
    dx, dy, dz = dims
    must, may = np.zeros(dx * dy * dz, bool), np.zeros(dx * dy * dz, bool)
    p, rad = np.asarray(p, F64), np.asarray(rad, F64)
    base = np.rint(p).astype(np.int64)
    R = np.ceil(rad + eps + 0.5).astype(np.int64)
    for r in np.unique(R):
        o = np.arange(-r, r + 1)
        off = np.stack(np.meshgrid(o, o, o, indexing="ij"), -1).reshape(-1, 3)
        sel = np.nonzero(R == r)[0]
        chunk = max(1, (1 << 21) // off.shape[0])
        for c in range(0, sel.size, chunk):
            i = sel[c:c + chunk]
            k = base[i, None, :] + off[None]
            d = np.sqrt(((k - p[i, None, :]) ** 2).sum(-1))
            inb = (k >= 0).all(-1) & (k[..., 0] < dx) & (k[..., 1] < dy) & (k[..., 2] < dz)
            flat = (k[..., 2] * dy + k[..., 1]) * dx + k[..., 0]
            must[flat[inb & (d < (rad[i] - eps)[:, None])]] = True
            may[flat[inb & (d <= (rad[i] + eps)[:, None])]] = True
    return must.reshape(dz, dy, dx), may.reshape(dz, dy, dx)


def spec_l1(marked):
    """Exact L1 distance transform (voxels, saturated at 255) of a bool volume: two sweeps per axis."""
    d = np.where(marked, 0, 255).astype(np.int32)
    for ax in range(d.ndim):
        v = np.moveaxis(d, ax, 0)
        for k in range(1, v.shape[0]):
            np.minimum(v[k], v[k - 1] + 1, out=v[k])
        for k in range(v.shape[0] - 2, -1, -1):
            np.minimum(v[k], v[k + 1] + 1, out=v[k])
    return np.minimum(d, 255).astype(np.uint8)


def unpack_bits(words, dims):
    """The bitmap's words (voxel b in bit b & 31 of word b >> 5) -> (bool [dz, dy, dx], the bits at and beyond n_vox)."""
    dx, dy, dz = dims
    flat = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    return flat[:dx * dy * dz].reshape(dz, dy, dx).astype(bool), flat[dx * dy * dz:]


def pack_bits(marked, n_words):
    flat = np.zeros(n_words * 32, np.uint8)
    flat[:marked.size] = marked.reshape(-1)
    return np.packbits(flat, bitorder="little").view(np.int32)


def spec_lookup(pv, dims, marked, dist, valid=True):
    """occ_lookup at points pv (..., 3) in voxel units relative to the box's corner: -> (marked, dist); outside the box, and on an
    invalid bitmap, a point counts as marked with distance 0."""
    pv = np.asarray(pv, F64)
    k = np.floor(pv).astype(np.int64)
    inside = (pv >= 0).all(-1) & (k[..., 0] < dims[0]) & (k[..., 1] < dims[1]) & (k[..., 2] < dims[2])
    if not valid:
        inside = np.zeros_like(inside)
    kc = np.where(inside[..., None], k, 0)
    mk = np.where(inside, marked[kc[..., 2], kc[..., 1], kc[..., 0]], True)
    dd = np.where(inside, dist[kc[..., 2], kc[..., 1], kc[..., 0]], 0)
    return mk, dd, inside


def spec_segments(o, d, t0, t1, dims, dist, sub=SUB, deep=DEEP):
    """Segments o + d t, t in [t0, t1] (voxel units relative to the box's corner), sampled every 1 / sub of a voxel.  Per ray:
    empty (t0 >= t1), inside (every sample in the box), dmin (smallest distance byte under a sample in the box; 255 without one),
    dmin_deep (the same over the samples deeper than `deep` inside their voxel), end_out (an end outside the box), face (distance of
    the ends to the nearest box face, voxels)."""
    o, d, t0, t1 = (np.asarray(a, F64) for a in (o, d, t0, t1))
    n = o.shape[0]
    res = dict(empty=~(t0 < t1), inside=np.zeros(n, bool), dmin=np.full(n, 255), dmin_deep=np.full(n, 255), end_out=np.zeros(n, bool),
               face=np.full(n, np.inf))
    dimv = np.asarray(dims, F64)
    live = np.nonzero(~res["empty"])[0]
    for e in (t0, t1):
        pe = o[live] + d[live] * e[live, None]
        res["end_out"][live] |= ~((pe >= 0) & (pe < dimv)).all(-1)
        res["face"][live] = np.minimum(res["face"][live], np.minimum(np.abs(pe), np.abs(pe - dimv)).min(-1))
    cnt = np.zeros(n, np.int64)
    cnt[live] = np.ceil(np.linalg.norm(d[live], axis=-1) * (t1 - t0)[live] * sub).astype(np.int64) + 1
    order = live[np.argsort(cnt[live])]
    for c in range(0, order.size, 256):
        i = order[c:c + 256]
        width = int(cnt[i].max())
        u = np.arange(width, dtype=F64)[None, :] / np.maximum(cnt[i] - 1, 1)[:, None]
        ok = u <= 1.0
        t = t0[i, None] + (t1 - t0)[i, None] * np.minimum(u, 1.0)
        pv = o[i, None, :] + d[i, None, :] * t[..., None]
        _, dd, ins = spec_lookup(pv, dims, np.zeros(dist.shape, bool), dist)
        fr = pv - np.floor(pv)
        dp = (np.minimum(fr, 1.0 - fr).min(-1) > deep) & ins
        res["inside"][i] = (ins | ~ok).all(-1)
        res["dmin"][i] = np.where(ins & ok, dd, 255).min(-1)
        res["dmin_deep"][i] = np.where(dp & ok, dd, 255).min(-1)
    return res


def spec_classify(valid, marked, dist, surf, conv, sigma, nearest=None):
    """k_tier_classify + k_tier_promote.  valid, marked, conv [n, S] bool, dist, sigma [n, S], surf [n] bool (conv / sigma: the
    sample's convergence and density IF it is evaluated in phase 1); nearest [n]: the nearest witness where the caller knows better
    than the smallest (dist, index).  -> final state [n, S] (TS_*), ray tier [n], witness ray [n]."""
    n, S = valid.shape
    state = np.where(valid, np.where(marked | surf[:, None], TS_PHASE1, TS_PENDING), TS_NONE)
    pend = state == TS_PENDING
    wit_ray = ~surf & ~(state == TS_PHASE1).any(-1) & pend.any(-1)
    key = np.where(pend, dist.astype(np.int64) * 65536 + np.arange(S)[None, :], 1 << 40)
    near = key.argmin(-1) if nearest is None else nearest
    for r in np.nonzero(wit_ray)[0]:
        for s in (near[r], S // 4, (3 * S) // 4):
            if pend[r, s]:
                state[r, s] = TS_PHASE1
    p1 = state == TS_PHASE1
    ok = p1 & conv
    promote = ~surf & ((ok & (sigma > 0)).any(-1) | ~ok.any(-1))
    state = np.where((state == TS_PENDING) & promote[:, None], TS_PHASE2, state)
    return state, np.where(surf, 1, np.where(promote, 2, 0)), wit_ray


# =====================================================================================================================
# the restatement against something more naive (CPU)
# =====================================================================================================================
def _brute_l1(marked):
    idx = np.stack(np.nonzero(np.ones(marked.shape, bool)), -1)
    src = np.stack(np.nonzero(marked), -1)
    if src.shape[0] == 0:
        return np.full(marked.shape, 255, np.uint8)
    d = np.abs(idx[:, None, :] - src[None, :, :]).sum(-1).min(-1)
    return np.minimum(d, 255).reshape(marked.shape).astype(np.uint8)


def test_spec_l1_against_brute_force():
    rng = np.random.RandomState(0)
    shapes = [(5, 7, 9), (9, 7, 5), (1, 1, 6), (3, 4, 4), (2, 9, 3)] + [tuple(rng.randint(1, 10, 3) % np.array([6, 8, 10]) + 1) for _ in range(12)]
    for shp in shapes:
        for density in (0.0, 0.02, 0.2, 0.9, 1.0):
            m = rng.rand(*shp) < density
            assert np.array_equal(spec_l1(m), _brute_l1(m)), (shp, density)
        one = np.zeros(shp, bool)
        one[tuple(rng.randint(0, s) for s in shp)] = True
        assert np.array_equal(spec_l1(one), _brute_l1(one)), shp
    assert bool((spec_l1(np.zeros((5, 7, 9), bool)) == 255).all())
    far = np.zeros((1, 1, 600), bool)
    far[0, 0, 0] = True                                    # saturation
    assert np.array_equal(spec_l1(far)[0, 0], np.minimum(np.arange(600), 255))


def test_spec_bits_roundtrip():
    rng = np.random.RandomState(1)
    m = rng.rand(3, 4, 33) < 0.3
    words = pack_bits(m, 16)
    back, tail = unpack_bits(words, (33, 4, 3))
    assert np.array_equal(back, m) and not tail.any()
    b = (2 * 4 + 1) * 33 + 32                              # voxel (x 32, y 1, z 2): bit b & 31 of word b >> 5
    assert bool((int(np.uint32(words[b >> 5])) >> (b & 31)) & 1) == bool(m[2, 1, 32])


def test_spec_mark_against_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(2)
    dims = (20, 17, 13)
    p = rng.rand(60, 3) * (np.array(dims) + 6.0) - 3.0       # some images outside the box: their balls are clipped at its faces
    rad = np.array([1.3, 2.9, 5.25])[rng.randint(0, 3, 60)]
    rad[:4] = [0.2, 0.49, 0.51, 9.7]                           # a ball that holds no centre, and one over most of the box
    must, may = spec_mark(p, rad, dims, MARK_EPS)
    zz, yy, xx = np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij")
    centres = np.stack([xx, yy, zz], -1).reshape(-1, 3).astype(F64)
    tree = cKDTree(centres)
    for vol, r in ((must, rad - MARK_EPS - 1e-12), (may, rad + MARK_EPS)):
        want = np.zeros(centres.shape[0], bool)
        for hits in tree.query_ball_point(p, r):
            want[hits] = True
        assert np.array_equal(vol.reshape(-1), want)
    assert must.any() and (may & ~must).sum() < 0.01 * must.sum() and not must.all()
    lone = spec_mark(np.array([[3.5, 3.5, 3.5]]), np.array([0.2]), dims, MARK_EPS)      # a ball that holds no centre marks nothing
    assert not lone[1].any()


def _hand_grid():
    """12 x 10 x 8 voxels with a marked 3 x 3 x 3 block at x 4..6, y 3..5, z 2..4."""
    marked = np.zeros((8, 10, 12), bool)
    marked[2:5, 3:6, 4:7] = True
    return (12, 10, 8), marked, spec_l1(marked)


def test_spec_segments_against_dense_sampling():
    dims, marked, dist = _hand_grid()
    rays = [  # origin, direction (voxels per unit t), t0, t1 -> expected (inside, dmin)
        ((0.5, 4.5, 3.5), (1, 0, 0), 0.0, 11.0, (True, 0)),        # through the block along x
        ((0.5, 6.5, 3.5), (1, 0, 0), 0.0, 11.0, (True, 1)),        # grazing at one voxel
        ((0.5, 7.5, 3.5), (1, 0, 0), 0.0, 11.0, (True, 2)),
        ((0.5, 8.5, 3.5), (1, 0, 0), 0.0, 11.0, (True, 3)),
        ((5.5, 9.5, 0.5), (0, 0, 1), 0.0, 7.0, (True, 4)),         # along z, past the block
        ((5.5, 0.5, 3.5), (0, 1, 0), 0.0, 20.0, (False, 0)),       # leaves the box through y
        ((-2.0, 4.5, 3.5), (1, 0, 0), 0.0, 4.0, (False, 2)),       # starts outside, ends in voxel x = 2
        ((0.25, 0.25, 0.25), (1, 0.7, 0.55), 0.0, 11.0, (True, 0)),   # a diagonal through the block
        ((0.5, 9.5, 7.5), (1, 0, 0), 0.0, 11.0, (True, 7)),        # along the far edge of the box
        ((11.5, 0.5, 0.5), (-1, 0, 0), 0.0, 11.0, (True, 5)),      # backwards along x
    ]
    o, d, t0, t1 = (np.array([r[k] for r in rays], F64) for k in range(4))
    coarse = spec_segments(o, d, t0, t1, dims, dist)
    dense = spec_segments(o, d, t0, t1, dims, dist, sub=1024)
    for k, r in enumerate(rays):
        assert (bool(coarse["inside"][k]), int(coarse["dmin"][k])) == r[4], (k, coarse["inside"][k], coarse["dmin"][k])
    for key in ("inside", "dmin", "end_out", "empty"):
        assert np.array_equal(coarse[key], dense[key]), key
    assert list(coarse["end_out"]) == [False] * 5 + [True, True, False, False, False]
    empty = spec_segments(o[:2], d[:2], np.array([1.0, 2.0]), np.array([1.0, 1.0]), dims, dist)
    assert empty["empty"].all() and not empty["inside"].any() and (empty["dmin"] == 255).all()
    # a point on a face belongs to the voxel above it, as floor() says; the ray in the plane y = 6 sees the voxels y = 6
    plane = spec_segments(np.array([[0.5, 6.0, 3.5]]), np.array([[1.0, 0, 0]]), np.zeros(1), np.full(1, 11.0), dims, dist)
    assert int(plane["dmin"][0]) == 1 and int(plane["dmin_deep"][0]) == 255
    mk, dd, ins = spec_lookup(np.array([[4.0, 3.0, 2.0], [3.999, 3.0, 2.0], [-0.0, 0.0, 0.0], [12.0, 1, 1], [1, -1e-9, 1]]), dims, marked, dist)
    assert list(mk) == [True, False, False, True, True] and list(dd) == [0, 1, 9, 0, 0] and list(ins) == [True, True, True, False, False]
    assert spec_lookup(np.array([[0.5, 0.5, 0.5]]), dims, marked, dist, valid=False)[0][0]


def test_spec_classifier_on_hand_written_rays():
    S = 8
    T, F = True, False
    rows = []   # valid, marked, dist, surf, conv, sigma -> state, tier, witness ray

    def ray(valid, marked, dist, surf, conv, sigma, state, tier, wit):
        rows.append((valid, marked, dist, surf, conv, sigma, state, tier, wit))

    z8, a8 = [0] * S, [T] * S
    ray(a8, [F, F, T, T, F, F, F, F], [2, 1, 0, 0, 1, 2, 3, 4], T, a8, z8, [1] * S, 1, F)                           # a surface ray: every valid sample
    ray([T, T, T, T, T, T, F, F], [F] * S, [3] * S, T, [F] * S, z8, [1, 1, 1, 1, 1, 1, 0, 0], 1, F)                 # ... and only the valid ones
    ray(a8, [F, F, F, T, F, F, F, F], [3, 2, 1, 0, 1, 2, 3, 4], F, a8, [0, 0, 0, .5, 0, 0, 0, 0], [3, 3, 3, 1, 3, 3, 3, 3], 2, F)   # density > 0: promoted
    ray(a8, [F, F, F, T, F, F, F, F], [3, 2, 1, 0, 1, 2, 3, 4], F, a8, [9, 9, 9, 0, 9, 9, 9, 9], [2, 2, 2, 1, 2, 2, 2, 2], 0, F)   # density +0: stays
    ray(a8, [F, F, F, T, F, F, F, F], [3, 2, 1, 0, 1, 2, 3, 4], F, [T, T, T, F, T, T, T, T], [9] * S, [3, 3, 3, 1, 3, 3, 3, 3], 2, F)  # none converged
    ray(a8, [F] * S, [5, 4, 4, 6, 7, 8, 9, 9], F, a8, z8, [2, 1, 1, 2, 2, 2, 1, 2], 0, T)                             # witnesses: (4, index 1), S/4 = 2, 3S/4 = 6
    ray(a8, [F] * S, [5, 4, 4, 6, 7, 8, 9, 9], F, [T, F, F, T, T, T, F, T], z8, [3, 1, 1, 3, 3, 3, 1, 3], 2, T)       # no witness converged
    ray(a8, [F] * S, [5, 4, 4, 6, 7, 8, 9, 9], F, [F, F, T, F, F, F, F, F], [0, 0, 1e-9, 0, 0, 0, 0, 0], [3, 1, 1, 3, 3, 3, 1, 3], 2, T)  # a witness with density
    ray([T, T, F, T, T, T, F, T], [F] * S, [9, 9, 0, 9, 9, 3, 0, 9], F, a8, z8, [2, 2, 0, 2, 2, 1, 0, 2], 0, T)       # S/4 and 3S/4 invalid: one witness
    ray([F] * S, [F] * S, [9] * S, F, a8, [9] * S, [0] * S, 2, F)                                                   # no valid sample: nothing converged
    ray([F, F, F, F, F, F, F, T], [F] * S, [0, 0, 0, 0, 0, 0, 0, 200], F, a8, z8, [0, 0, 0, 0, 0, 0, 0, 1], 0, T)     # the only pending sample
    ray(a8, [T] * S, [0] * S, F, a8, z8, [1] * S, 0, F)                                                             # all marked, all +0
    cols = list(zip(*rows))
    arr = lambda k, dt: np.array(cols[k], dt)
    state, tier, wit = spec_classify(arr(0, bool), arr(1, bool), arr(2, np.int64), arr(3, bool), arr(4, bool), arr(5, F64))
    for r in range(len(rows)):
        assert list(state[r]) == rows[r][6] and int(tier[r]) == rows[r][7] and bool(wit[r]) == rows[r][8], r


def test_spec_refinement_and_slopes_on_a_linear_field():
    """sdf = g . x + c: every edge slope is |g_a|, the fine pairs' steepest slope |g| (along g's octant diagonal at most), the minimum
    corner is known in closed form."""
    nc, L = 5, 1.5
    g, c0 = np.array([0.5, -2.0, 1.0]), 0.3
    pts = spec_lattice(nc, L)
    assert pts.shape == (125, 3) and np.allclose(pts[(1 * nc + 2) * nc + 3], [-0.75, 0.0, 0.75])
    q, lip, edge = spec_refine(pts @ g + c0, nc, L)
    step = 0.75
    assert np.allclose(lip, max(1.5, 1.25 * 2.0)) and edge.sum() == 64 - 8 and not edge[1:3, 1:3, 1:3].any()
    corner = spec_lattice(nc, L).reshape(nc, nc, nc, 3)[:-1, :-1, :-1]          # the cells' low corners
    mn = corner @ g + c0 + step * (0 - 2.0 + 0)                                   # g_y < 0: the minimum sits at the high-y corner
    assert np.allclose(q, mn - 2.5 * step * SQ3H)
    cells = np.array([[0, 0, 0], [1, 2, 3]])
    fine = spec_fine_lattice(cells, nc, L)
    assert np.allclose(fine[1, 0], -L + step * np.array([1, 2, 3]) + step / 6) and np.allclose(fine[1, 26] - fine[1, 0], step * 2 / 3)
    assert np.allclose(fine[1, 5] - fine[1, 0], step / 3 * np.array([0, 1, 2]))
    cl = spec_cell_lip(np.array([2.5, 1.5]), np.array([True, False]), fine @ g + c0, nc, L)
    steepest = max(abs(g @ (a - b)) / np.linalg.norm(a - b) for a in _OFF27 for b in _OFF27 if (a != b).any())
    assert np.allclose(cl, [-2.5, 1.25 * steepest]) and steepest <= np.linalg.norm(g) + 1e-12
    qs = spec_select_quantity((fine @ g + c0).reshape(-1), cl, nc, L)
    assert np.allclose(qs[:27], (fine[0] @ g + c0) - 2.5 * step / 3 * SQ3H)
    ok = np.zeros((2, 27), bool)
    ok[0, [0, 13]] = True                                                         # one pair: the body diagonal's half
    st = spec_pair_max(fine * np.array([1.0, 2.0, 3.0]), ok, step / 3)
    assert np.allclose(st, [np.sqrt(1 + 4 + 9) / np.sqrt(3), 0.0])
    x, mag = spec_unnormalize(np.array([[0.0, 1.0, -1.0]]), -1.0, 1.0, np.array([0.1, 0.2, 0.3]))
    assert np.allclose(x, [[0.1, 1.3, -0.8]]) and np.allclose(mag, [[1.1, 2.2, 1.0]])


# =====================================================================================================================
# GPU: the build
# =====================================================================================================================
SUBJECTS = {"zju377_mono": 5, "h36m": 3, "wide": 0}      # subject -> frame ('wide': zju377_mono with fixture F17's skinning MLP)
_ORACLE = {}


def oracle_frame(scene, subject, frame_idx=None, H=64):
    """(fp32 Frame, float64 Frame, model config) of a subject's frame from the oracle."""
    frame_idx = SUBJECTS[subject] if frame_idx is None else frame_idx
    key = (subject, frame_idx)
    if key not in _ORACLE:
        from arah_release_amd import config
        if subject == "wide":
            model, cfg = config.build_synthetic_model("zju377_mono", device="cpu")
            config.widen_skinning_(model, float(golden("f17_wide_skinning.npz")["scale"]))
        else:
            model, cfg = get_model(subject)
        fr = O.frame_from_model(model, scene.make_inputs(H, H, frame_idx=frame_idx))
        _ORACLE[key] = (fr, O.frame_as(fr, torch.float64), cfg)
    return _ORACLE[key]


def header_of(info_words):
    w = np.ascontiguousarray(info_words).astype(np.int32)
    f = w.view(np.float32)
    return dict(origin=f[0:3].astype(F64), v=float(f[3]), inv_v=float(f[4]), dims=tuple(int(x) for x in w[5:8]), n_vox=int(w[8]),
                valid=int(w[9]), n_cells=int(w[10]), n_fine=int(w[11]), n_sel=int(w[12]), overflow=int(w[13]), band_m=float(f[14]),
                lip_pose=float(f[15]), lip_pose_bits=int(w[15]), v32=f[3], band32=f[14])


def build_occupancy(hip, frame, dev):
    """One build into a canary-filled buffer on a workspace of its own -> (ws, occ, host copy of the raw bytes)."""
    ws = hip.Workspace(dev)
    ws.occ = torch.full((int(hip.load_library().arah_occupancy_bytes()),), CANARY, dtype=torch.uint8, device=dev)
    occ = ws.occupancy(frame)
    torch.cuda.synchronize()
    assert occ is ws.occ
    return ws, occ, occ.cpu().numpy().copy()


def host_view(hip, raw):
    layout, total = hip.occupancy_layout()
    np_dt = {torch.int32: np.int32, torch.uint8: np.uint8, torch.float32: np.float32}
    return {name: raw[off:off + nbytes].view(np_dt[dt]).reshape(shape) for name, off, nbytes, dt, shape in layout}


def context_of(scene, subject, eng, fr=None):
    from arah_release_amd import hip
    dev = torch.device("cuda:0")
    if fr is None:
        fr, fr64, _ = oracle_frame(scene, subject)
    else:
        fr64 = O.frame_as(fr, torch.float64)
    frame = hip_frame(fr, dev, eng)
    ws, occ, raw = build_occupancy(hip, frame, dev)
    a = host_view(hip, raw)
    h = header_of(a["info"])
    marked, tail = unpack_bits(a["bits"], h["dims"]) if 0 < h["n_vox"] <= hip.OCC_MAX_VOX else (None, None)
    scale = (fr.coord_max - fr.coord_min) * 1.1 / 2.0
    return dict(hip=hip, dev=dev, fr=fr, fr64=fr64, frame=frame, ws=ws, occ=occ, raw=raw, a=a, h=h, marked=marked, tail=tail,
                scale=scale, band_n=h["band_m"] / scale, tag="%s %s" % (subject, eng), subject=subject, eng=eng)


@pytest.fixture(scope="module", params=[(s, e) for s in SUBJECTS for e in ENGINES], ids=lambda p: "%s-%s" % p)
def built(request, scene):
    return context_of(scene, *request.param)


@gpu
def test_layout_size_is_the_librarys():
    from arah_release_amd import hip
    assert hip.occupancy_layout()[1] == int(hip.load_library().arah_occupancy_bytes())


@gpu
def test_build_chains_to_the_tested_kernels(built):
    """csdf, fsdf and sel_bar are outputs of the kernels tests/test_pointwise_f64.py holds to float64: bit for bit the public entries'."""
    c, hip = built, built["hip"]
    v = hip.occupancy_view(c["occ"])
    h = c["h"]
    ws2 = hip.Workspace(c["dev"])
    csdf, _, _ = hip.sdf_eval(c["frame"], ws2, v["cpts"])
    assert torch.equal(csdf.view(torch.int32), v["csdf"].view(torch.int32)), int((csdf != v["csdf"]).sum())
    nf, ns = h["n_fine"], h["n_sel"]
    fsdf, _, _ = hip.sdf_eval(c["frame"], ws2, v["fnorm"][:nf])
    assert torch.equal(fsdf.view(torch.int32), v["fsdf"][:nf].view(torch.int32)), int((fsdf != v["fsdf"][:nf]).sum())
    _, xb, _ = hip.skin_lbs(c["frame"], ws2, v["sel_raw"][:ns])
    assert torch.equal(xb.contiguous().view(torch.int32), v["sel_bar"][:ns].view(torch.int32)), int((xb != v["sel_bar"][:ns]).any(-1).sum())


def _restated_headers(fr, beta):
    """k_occ_begin after the nearest-vertex grid's box (vertices' box + 0.08 m, cell side from cbrtf): fp32 arithmetic restated with
    numpy's; cbrtf is good to an ulp, so the grid's cell side and its two fp32 neighbours are all admitted."""
    f = np.float32
    verts = fr.verts.numpy().astype(f)
    lo, hi = verts.min(0) - f(0.08), verts.max(0) + f(0.08)
    ext = (hi - lo).astype(f)
    h0 = max(f(np.cbrt(f(f(ext[0] * ext[1]) * ext[2]) / f(48000.0))), f(0.02))
    out = []
    for h in (np.nextafter(h0, f(0)), h0, np.nextafter(h0, f(1))):
        h = f(h)
        while True:
            gd = np.maximum(np.ceil(ext / h), 1)
            if gd.prod() <= 65536:
                break
            h = f(h * f(1.1))
        e = (gd.astype(f) * h).astype(f)
        v = f(0.015)
        for _ in range(32):
            if np.prod(np.ceil(e.astype(F64) / F64(v))) <= (1 << 22):
                break
            v = f(v * f(1.1))
        dims = tuple(int(x) for x in np.maximum(1, np.ceil((e / v).astype(f))))
        out.append((dims, float(v)))
    b = f(min(max(abs(f(beta)), f(1e-6)), f(1e6)))
    return lo, out, float(f(18.0) * b)


@gpu
def test_build_header_and_lattice(built):
    c, h, a, hip = built, built["h"], built["a"], built["hip"]
    lo, cands, band_m = _restated_headers(c["fr"], c["fr"].beta)
    assert np.array_equal(h["origin"].astype(np.float32), lo)
    assert (h["dims"], h["v"]) in cands, (h["dims"], h["v"], cands)
    assert h["n_vox"] == int(np.prod(h["dims"])) <= hip.OCC_MAX_VOX and h["inv_v"] == float(np.float32(1.0) / h["v32"])
    assert h["band_m"] == band_m
    hi = c["fr"].verts.numpy().max(0).astype(F64) + 0.08          # the box covers the vertices' box and its margin
    assert bool((h["origin"] + np.array(h["dims"]) * h["v"] >= hi - 1e-6).all()) and min(h["dims"]) >= 4
    assert h["n_fine"] == 27 * h["n_cells"] and h["overflow"] == 0 and h["valid"] == 1
    assert 0 < h["n_cells"] <= hip.OCC_MAX_CELLS and 0 < h["n_sel"] <= h["n_fine"]
    # fp32 evaluates -L + step * i with one or two roundings: within an ulp of 1.5 of the float64 lattice
    assert float(np.abs(a["cpts"].astype(F64) - spec_lattice(hip.OCC_NC, hip.OCC_L)).max()) <= 2.0 ** -22


def _refined_cells(c):
    """Coarse cell (cx, cy, cz) of every slot, recovered from its first fine point: x = -L + step (cx + 1 / 6)."""
    hip, h = c["hip"], c["h"]
    step = 2.0 * hip.OCC_L / (hip.OCC_NC - 1)
    first = c["a"]["fnorm"][:h["n_fine"]].reshape(-1, 27, 3)[:, 0, :].astype(F64)
    t = (first + hip.OCC_L) / step - 1.0 / 6.0
    cells = np.rint(t).astype(np.int64)
    assert float(np.abs(t - cells).max()) < 1e-4 and cells.min() >= 0 and cells.max() <= hip.OCC_NC - 2
    return cells


@gpu
def test_build_refinement(built):
    c, h, a, hip = built, built["h"], built["a"], built["hip"]
    nc, L, m = hip.OCC_NC, hip.OCC_L, hip.OCC_NC - 1
    assert bool(np.isfinite(a["csdf"]).all())
    q, lip, edge = spec_refine(a["csdf"], nc, L)
    thr = c["band_n"]
    shell = np.abs(q - thr) <= SHELL_REL * abs(thr)
    want = q <= thr
    cells = _refined_cells(c)
    flat = (cells[:, 0] * m + cells[:, 1]) * m + cells[:, 2]
    assert np.unique(flat).size == flat.size == h["n_cells"]                     # no cell twice
    got = np.zeros(m ** 3, bool)
    got[flat] = True
    got = got.reshape(m, m, m)
    wrong = (got != want) & ~shell
    assert not wrong.any(), "%d cells differ from the restated set, e.g. %s (q - band_n %s)" % (
        wrong.sum(), np.argwhere(wrong)[:3].tolist(), (q - thr)[wrong][:3])
    report("refinement", c["tag"], int(shell.sum()), h["n_cells"], CAP)
    nf = h["n_fine"]
    # the sub-lattice: fp32 sums of three terms below 1.5, each rounded once
    assert float(np.abs(a["fnorm"][:nf].astype(F64).reshape(-1, 27, 3) - spec_fine_lattice(cells, nc, L)).max()) <= 2.0 ** -21
    assert np.array_equal(a["iota"][:nf], np.arange(nf, dtype=np.int32))
    ci = (cells[:, 0], cells[:, 1], cells[:, 2])
    want_lip = spec_cell_lip(lip[ci], edge[ci], a["fsdf"][:nf].reshape(-1, 27), nc, L)
    got_lip = a["cell_lip"][:h["n_cells"]].astype(F64)
    rel = np.abs(got_lip - want_lip) / np.abs(want_lip)
    assert float(rel.max()) <= 1e-5, (float(rel.max()), int(rel.argmax()))
    assert bool((np.abs(got_lip) >= 1.5).all()) and bool(((got_lip < 0) == edge[ci]).all())


@gpu
def test_build_selection(built):
    c, h, a, hip = built, built["h"], built["a"], built["hip"]
    nf, ns, ncell = h["n_fine"], h["n_sel"], h["n_cells"]
    assert bool(np.isfinite(a["fsdf"][:nf]).all())
    q = spec_select_quantity(a["fsdf"][:nf], a["cell_lip"][:ncell], hip.OCC_NC, hip.OCC_L)
    thr = c["band_n"]
    shell = np.abs(q - thr) <= SHELL_REL * abs(thr)
    want = ~(q > thr)
    sel_of, sel_idx = a["sel_of"], a["sel_idx"][:ns]
    got = sel_of[:nf] >= 0
    wrong = (got != want) & ~shell
    assert not wrong.any(), "%d fine points differ from the restated selection, e.g. %s" % (wrong.sum(), np.nonzero(wrong)[0][:3].tolist())
    report("selection", c["tag"], int(shell.sum()), ns, CAP)
    assert int(got.sum()) == ns and bool((sel_of[nf:] == -1).all()) and bool((sel_of[:nf][~got] == -1).all())
    assert np.array_equal(np.sort(sel_idx), np.nonzero(got)[0]) and np.array_equal(sel_of[sel_idx], np.arange(ns, dtype=np.int32))
    fr = c["fr"]
    raw64, mag = spec_unnormalize(a["fnorm"][sel_idx], F64(np.float32(fr.coord_min)), F64(np.float32(fr.coord_max)), fr.center.numpy().astype(F64))
    # 2 ulp -- of the largest term of the fp32 sum (p / 2 + 0.5) 1.1 rng + cmin - pad + center: no sum is better than its terms' spacing
    ulp = np.spacing(mag.astype(np.float32)).astype(F64)
    err = np.abs(a["sel_raw"][:ns].astype(F64) - raw64) / ulp
    assert float(err.max()) <= 2.0, float(err.max())
    # a selected fine point in a boundary cell invalidates the bitmap; these three are valid
    assert not (got & (np.repeat(a["cell_lip"][:ncell], 27) < 0)).any()


def _stretch_inputs(c):
    hip, h, a = c["hip"], c["h"], c["a"]
    so = a["sel_of"][:h["n_fine"]].reshape(-1, 27)
    bar = a["sel_bar"][:h["n_sel"]].astype(F64)
    fs_m = 2.0 * hip.OCC_L / (hip.OCC_NC - 1) / 3.0 * c["scale"]
    return so, bar, fs_m


@gpu
def test_build_stretch(built):
    c, h, a = built, built["h"], built["a"]
    so, bar, fs_m = _stretch_inputs(c)
    want = spec_pair_max(bar[np.maximum(so, 0)], so >= 0, fs_m)
    got = a["cell_stretch"][:h["n_cells"]]
    assert bool(np.isfinite(got).all())
    rel = np.abs(got.astype(F64) - want) / np.maximum(want, 1e-30)
    assert float(rel[want > 0].max()) <= 1e-5 and bool((got[want == 0] == 0).all()), float(rel[want > 0].max())
    assert h["lip_pose_bits"] == int(got.max().view(np.int32)) and h["lip_pose"] > 0.9     # atomicMax over the same floats
    print("occupancy_spec | stretch      %-24s cells %d, measured max %.3f, cells above 1.2 (the radius floor): %d" % (
        c["tag"], h["n_cells"], h["lip_pose"], int((got > 1.2).sum())))


def _mark_inputs(c):
    """The images in voxel units relative to the voxel centres and the kernel's own radius per selected point."""
    hip, h, a, fr = c["hip"], c["h"], c["a"], c["fr"]
    ns = h["n_sel"]
    half_m = 2.0 * hip.OCC_L / (hip.OCC_NC - 1) / 3.0 * SQ3H * c["scale"]
    lip = np.maximum(1.5, 1.25 * a["cell_stretch"][a["sel_idx"][:ns] // 27].astype(F64))
    rad = (lip * half_m + F64(np.float32(1e-4))) * h["inv_v"] + SQ3H
    p = (a["sel_bar"][:ns].astype(F64) + fr.trans.numpy().astype(F64) - h["origin"]) * h["inv_v"] - 0.5
    return p, rad


@gpu
def test_build_marking(built):
    c, h = built, built["h"]
    p, rad = _mark_inputs(c)
    assert bool(np.isfinite(p).all())
    must, may = spec_mark(p, rad, h["dims"], MARK_EPS)
    marked = c["marked"]
    missing, extra = must & ~marked, marked & ~may
    assert not missing.any(), "%d voxels inside a ball are unmarked, e.g. (z, y, x) %s" % (missing.sum(), np.argwhere(missing)[:3].tolist())
    assert not extra.any(), "%d marked voxels lie outside every ball, e.g. (z, y, x) %s" % (extra.sum(), np.argwhere(extra)[:3].tolist())
    assert not c["tail"].any(), "bits at or beyond n_vox are set"
    report("marking", c["tag"], int((may & ~must).sum()), int(marked.sum()), CAP)
    print("occupancy_spec | marking      %-24s dims %s, marked %d of %d voxels (%.1f %%), radius %.2f .. %.2f voxels" % (
        c["tag"], h["dims"], marked.sum(), marked.size, 100.0 * marked.mean(), rad.min(), rad.max()))


@gpu
def test_build_distances(built):
    c, h = built, built["h"]
    dx, dy, dz = h["dims"]
    got = c["a"]["dist"][:h["n_vox"]].reshape(dz, dy, dx)
    want = spec_l1(c["marked"])
    assert np.array_equal(got, want), "%d voxels differ, e.g. (z, y, x) %s" % ((got != want).sum(), np.argwhere(got != want)[:3].tolist())


def _assert_canary(c):
    hip, h, a, raw = c["hip"], c["h"], c["a"], c["raw"]
    layout, total = hip.occupancy_layout()
    assert raw.size == total
    end = 0
    for name, off, nbytes, _, _ in layout:
        assert bool((raw[end:off] == CANARY).all()), "the gap before %s was written" % name
        end = off + nbytes
    assert bool((raw[end:] == CANARY).all())
    can32 = np.frombuffer(bytes([CANARY] * 4), np.int32)[0]
    tails = dict(dist=h["n_vox"], fsdf=h["n_fine"], fnorm=h["n_fine"], sel_raw=h["n_sel"], sel_bar=h["n_sel"], sel_idx=h["n_sel"])
    for name, n in tails.items():
        t = a[name][n:]
        t = t if t.dtype == np.uint8 else t.view(np.int32)
        assert bool((t == (CANARY if t.dtype == np.uint8 else can32)).all()), "%s was written beyond %d" % (name, n)


@gpu
def test_build_touches_nothing_else_and_repeats(built):
    c, hip = built, built["hip"]
    _assert_canary(c)
    _, _, raw2 = build_occupancy(hip, c["frame"], c["dev"])
    b = host_view(hip, raw2)
    h2 = header_of(b["info"])
    assert np.array_equal(b["bits"], c["a"]["bits"]) and np.array_equal(b["dist"][:h2["n_vox"]], c["a"]["dist"][:c["h"]["n_vox"]])
    assert np.array_equal(b["info"][:14], c["a"]["info"][:14]) and h2["lip_pose_bits"] == c["h"]["lip_pose_bits"]


_FAT = {}


def fat_body_points(scene, subject):
    """Posed images (float64 oracle LBS + trans) of canonical points drawn uniformly in [-1.5, 1.5]^3 whose float64 oracle SDF in
    metres is <= 17.33 beta: the true band.  Independent of the engine and of every intermediate of the buffer."""
    if subject not in _FAT:
        fr, fr64, _ = oracle_frame(scene, subject)
        gen = torch.Generator().manual_seed(20260218)
        beta = min(max(abs(fr.beta), 1e-6), 1e6)
        keep, have, drawn = [], 0, 0
        while have < 2000 and drawn < 400000:
            x = (torch.rand(40000, 3, generator=gen, dtype=torch.float64) * 2.0 - 1.0) * 1.5
            drawn += x.shape[0]
            s = chunked(lambda q: O.sdf_forward(fr64, q, count=False)[0], x) * fr64.sdf_scale
            x = x[s <= 17.33 * beta]
            keep.append(x)
            have += x.shape[0]
        x = torch.cat(keep)
        xb, _ = chunked(lambda q: O.lbs_forward(fr64, q, count=False), O.unnormalize_points(fr64, x))
        _FAT[subject] = ((xb + fr64.trans).numpy(), drawn)
    return _FAT[subject]


@gpu
def test_build_is_sound_against_the_float64_oracle(built, scene):
    """Every point of the true posed fat body lies in a marked voxel or outside the bitmap's box, and the bitmap is not trivially full."""
    c, h = built, built["h"]
    pts, drawn = fat_body_points(scene, c["subject"])
    # the stopping rule is 2 000 points or 400 000 draws; the fat body fills ~0.47 % of the lattice's box (zju377_mono: 1 894 points
    # of 400 000 draws), so the draws may run out first -- a thousand points still look at every limb
    assert pts.shape[0] >= 2000 or (drawn >= 400000 and pts.shape[0] >= 1000), (pts.shape[0], drawn)
    mk, _, inside = spec_lookup((pts - h["origin"]) * h["inv_v"], h["dims"], c["marked"], c["a"]["dist"][:h["n_vox"]].reshape(c["marked"].shape))
    bad = ~mk
    print("occupancy_spec | soundness    %-24s %d fat-body points of %d draws, %d inside the box, %d in unmarked voxels; unmarked voxels %.1f %%" % (
        c["tag"], pts.shape[0], drawn, inside.sum(), bad.sum(), 100.0 * (1 - c["marked"].mean())))
    assert not bad.any(), "%d points of the posed fat body lie in unmarked voxels, e.g. %s" % (bad.sum(), pts[bad][:3].tolist())
    assert inside.sum() >= 0.9 * pts.shape[0]
    assert 1.0 - c["marked"].mean() >= 0.30


@pytest.fixture(scope="module", params=[(b, e) for b in ("ladder", 1.0) for e in ENGINES], ids=lambda p: "%s-%s" % p)
def swallowed(request, scene):
    """A frame whose beta is raised until the band swallows the lattice ('ladder': the first of 3e-2, 6e-2, 0.1, 0.3 that invalidates
    the bitmap; 1.0: every coarse cell is refined and the cell list overflows)."""
    how, eng = request.param
    fr, _, _ = oracle_frame(scene, "zju377_mono")
    for beta in ((3e-2, 6e-2, 0.1, 0.3, 1.0) if how == "ladder" else (how,)):
        c = context_of(scene, "zju377_mono beta %g" % beta, eng, fr=dataclasses.replace(fr, beta=beta))
        if c["h"]["valid"] == 0:
            return c
    raise AssertionError("no beta of the ladder invalidates the bitmap")


@gpu
def test_invalid_bitmap(swallowed):
    c, h, a, hip = swallowed, swallowed["h"], swallowed["a"], swallowed["hip"]
    print("occupancy_spec | invalid      %-24s n_cells %d n_sel %d overflow %d" % (c["tag"], h["n_cells"], h["n_sel"], h["overflow"]))
    assert h["valid"] == 0 and 0 < h["n_cells"] <= hip.OCC_MAX_CELLS and h["n_fine"] == 27 * h["n_cells"]
    assert not a["bits"].any()
    _assert_canary(c)
    lo = h["origin"]
    hi = lo + np.array(h["dims"]) * h["v"]
    rng = np.random.RandomState(4)
    pts = torch.from_numpy((lo - 0.2 + rng.rand(2000, 3) * (hi - lo + 0.4)).astype(np.float32)).to(c["dev"])
    st = hip.query_posed(c["frame"], c["ws"], pts, occ=c["occ"], want=())["state"]
    assert not bool((st == 2).any())
    if h["overflow"] == 0:
        q = spec_select_quantity(a["fsdf"][:h["n_fine"]], a["cell_lip"][:h["n_cells"]], hip.OCC_NC, hip.OCC_L)
        boundary = np.repeat(a["cell_lip"][:h["n_cells"]], 27) < 0
        clear = ~(q > c["band_n"]) & (np.abs(q - c["band_n"]) > SHELL_REL * abs(c["band_n"]))
        assert (boundary & clear).any()


# =====================================================================================================================
# GPU: hand-made bitmaps
# =====================================================================================================================
@pytest.fixture(scope="module")
def plain(scene):
    """A real frame and header (zju377_mono, split engine) for the tests that write their own bitmaps."""
    return context_of(scene, "zju377_mono", "split")


def hand_made(c, dims, marked, origin=(0.0, 0.0, 0.0), v=0.0625, valid=1):
    """A zeroed occupancy buffer with a hand-written header and bitmap; arah_occupancy_clear_box with an empty box (lo > hi) clears
    nothing and recomputes the distances.  -> (buffer, dist [dz, dy, dx] on the host)."""
    hip, dev = c["hip"], c["dev"]
    dx, dy, dz = dims
    n_vox = dx * dy * dz
    # what occ_distance's launch needs (its comment: no axis below four voxels AT the largest bitmap): every pair of axes has at
    # most kOccMaxVox / 4 lines.  Every grid here has four or more voxels per axis but the 105-voxel 5 x 7 x 3.
    assert max(dx * dy, dx * dz, dy * dz) <= hip.OCC_MAX_VOX // 4 and n_vox <= hip.OCC_MAX_VOX and marked.shape == (dz, dy, dx)
    buf = torch.zeros(hip.occupancy_layout()[1], dtype=torch.uint8, device=dev)
    view = hip.occupancy_view(buf)
    info = np.zeros(16, np.int32)
    f = info.view(np.float32)
    f[0:3], f[3], f[4] = origin, v, 1.0 / v
    info[5:8], info[8], info[9] = dims, n_vox, valid
    f[14], f[15] = c["h"]["band32"], 1.0
    view["info"].copy_(torch.from_numpy(info))
    view["bits"].copy_(torch.from_numpy(pack_bits(marked, hip.OCC_MAX_VOX // 32)))
    ws = hip.Workspace(dev)
    ws.occ = buf
    ws.occupancy_clear_box((1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    torch.cuda.synchronize()
    assert torch.equal(view["bits"].cpu(), torch.from_numpy(pack_bits(marked, hip.OCC_MAX_VOX // 32)))   # nothing was cleared
    return buf, view["dist"][:n_vox].cpu().numpy().reshape(dz, dy, dx)


def _grid_cases():
    rng = np.random.RandomState(7)
    out = {}
    for dims in ((5, 7, 3), (33, 4, 4), (64, 4, 4)):
        out["%dx%dx%d" % dims] = (dims, rng.rand(dims[2], dims[1], dims[0]) < 0.04)
    corner = np.zeros((4, 4, 600), bool)
    corner[3, 3, 599] = True
    out["600x4x4 corner"] = ((600, 4, 4), corner)
    sparse = np.zeros((1024, 1024, 4), bool)
    idx = rng.randint(0, sparse.size, 400)
    sparse.reshape(-1)[idx] = True
    out["4x1024x1024 sparse"] = ((4, 1024, 1024), sparse)
    out["empty"] = ((9, 6, 5), np.zeros((5, 6, 9), bool))
    out["full"] = ((9, 6, 5), np.ones((5, 6, 9), bool))
    return out


GRIDS = _grid_cases()


@gpu
@pytest.mark.parametrize("name", list(GRIDS))
def test_hand_made_distances(plain, name):
    """k_occ_dist_* at shapes no real frame gives: rows that meet and straddle word boundaries, saturation, the largest line count
    the launch covers, the empty and the full bitmap.  Exact."""
    dims, marked = GRIDS[name]
    _, got = hand_made(plain, dims, marked)
    want = spec_l1(marked)
    assert np.array_equal(got, want), "%d voxels differ, e.g. (z, y, x) %s" % ((got != want).sum(), np.argwhere(got != want)[:3].tolist())
    if name == "empty":
        assert bool((got == 255).all())
    if name == "full":
        assert not got.any()
    if name.startswith("600"):
        assert got[3, 3, 599] == 0 and got[0, 0, 0] == 255 and got[3, 3, 599 - 254] == 254


@gpu
def test_hand_made_lookup(plain):
    """occ_lookup through query_posed on a 9 x 6 x 5 checkerboard with exactly representable voxel centres: state 2 exactly where the
    point's voxel is unmarked, never outside the box or on an invalid bitmap."""
    c, hip, dev = plain, plain["hip"], plain["dev"]
    dims, v = (9, 6, 5), 0.0625
    origin = np.array([-0.25, 0.5, -0.125])
    zz, yy, xx = np.meshgrid(np.arange(5), np.arange(6), np.arange(9), indexing="ij")
    marked = ((xx + yy + zz) % 2).astype(bool)
    buf, _ = hand_made(c, dims, marked, origin=origin, v=v)
    centres = origin + (np.stack([xx, yy, zz], -1).reshape(-1, 3) + 0.5) * v
    q = lambda p, b=buf: hip.query_posed(c["frame"], c["ws"], torch.from_numpy(np.asarray(p, np.float32)).to(dev), occ=b, want=())["state"].cpu().numpy()
    assert np.array_equal(q(centres) == 2, ~marked.reshape(-1))
    free = centres[~marked.reshape(-1)]
    f32 = np.float32
    hi = origin + np.array(dims) * v
    for a in range(3):
        below, at = free.astype(f32).copy(), free.astype(f32).copy()
        below[:, a] = np.nextafter(f32(origin[a]), f32(-np.inf))
        at[:, a] = f32(hi[a])
        inside = free.astype(f32).copy()
        inside[:, a] = f32(origin[a])                    # exactly on the low face: inside, the voxel of index 0
        assert not (q(below) == 2).any() and not (q(at) == 2).any(), a
        k = np.floor((inside.astype(F64) - origin) / v).astype(int)
        assert np.array_equal(q(inside) == 2, ~marked[k[:, 2], k[:, 1], k[:, 0]]), a
    rng = np.random.RandomState(5)
    out = origin - 1.0 + rng.rand(4000, 3) * (hi - origin + 2.0)
    out = out[((out < origin) | (out >= hi)).any(-1)].astype(f32)
    out = out[((out.astype(F64) < origin) | (out.astype(F64) >= hi)).any(-1)]
    assert out.shape[0] > 3000 and not (q(out) == 2).any()
    dead, _ = hand_made(c, dims, marked, origin=origin, v=v, valid=0)
    assert not (q(centres, dead) == 2).any()


# =====================================================================================================================
# GPU: the ray skip and the classifier
# =====================================================================================================================
F7 = "f7_forward_zju377_mono_64x64_s64.npz"


def _render(c, cam, dirs, nf, S, cano):
    """One tiered hip.render of explicit rays and its rate-1 audit -> host arrays."""
    hip, dev = c["hip"], c["dev"]
    ws = c["ws"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    cam_t, d_t, nf_t = t(cam), t(dirs), t(nf)
    n = d_t.shape[0]
    samp = hip.Sampling(dev, S, 16, 16, cano, False)
    ws.ensure(n, S)
    ws.reset_counters()
    pose = torch.eye(4, device=dev)[:3].contiguous()
    with torch.no_grad():
        out = hip.render(c["frame"], ws, samp, cam_t, d_t, nf_t, pose, tiered=True)
        smp = ws.debug_samples(n, S, which=("z", "mask", "shaded", "state"))
        tier, _ = ws.tier_debug(n, S)
        torch.cuda.synchronize()
        ctr = ws.counters()
        hip.audit_result(hip.tier_audit(c["frame"], ws, samp, cam_t, d_t, nf_t, 0, 0))
        _, rtag = ws.tier_audit_debug(n, S)
        torch.cuda.synchronize()
    a = host_view(hip, ws.occ.cpu().numpy())
    h = header_of(a["info"])
    marked, _ = unpack_bits(a["bits"], h["dims"])
    dist = a["dist"][:h["n_vox"]].reshape(marked.shape)
    g = lambda x: x.cpu().numpy()
    return dict(n=n, S=S, conv=g(out[5]) != 0, z=g(smp["z"]).reshape(n, S), mask=g(smp["mask"]).reshape(n, S) != 0,
                sigma=g(smp["shaded"])[:, 3].reshape(n, S), state=g(smp["state"]).reshape(n, S), tier=g(tier), ctr=ctr,
                skipped=g(rtag) != 0, h=h, marked=marked, dist=dist)


@pytest.fixture(scope="module", params=ENGINES)
def f7_render(request, scene):
    """Fixture F7's 64 x 64 x 64 frame of zju377_mono rendered tiered through hip.render, from the oracle's frame."""
    g = golden(F7)
    H, S, fi = int(g["H"]), int(g["n_steps"]), int(g["frame_idx"])
    fr, _, cfg = oracle_frame(scene, "zju377_mono", fi, H)
    c = context_of(scene, "zju377_mono f7", request.param, fr=fr)
    inputs = scene.make_inputs(H, int(g["W"]), frame_idx=fi)
    cam = inputs["cam_loc"].numpy().reshape(1, 3)
    dirs, nf = inputs["ray_dirs"][0].numpy(), inputs["body_bounds_intersections"][0].numpy()
    c["cano"] = bool(cfg["model"]["cano_view_dirs"])
    c["rays"] = dict(cam=np.repeat(cam, dirs.shape[0], 0), dirs=dirs, nf=nf)
    c["r"] = _render(c, cam, dirs, nf, S, c["cano"])
    assert np.array_equal(c["r"]["marked"], c["marked"])          # the render built the fixture's bitmap again, bit for bit
    return c


def _judge_ray_skip(c, r, cam, dirs, nf, tag):
    h = r["h"]
    f32 = np.float32
    o = (np.asarray(cam, f32).astype(F64) - h["origin"]) * h["inv_v"]
    d = np.asarray(dirs, f32).astype(F64) * h["inv_v"]
    nf = np.asarray(nf, f32).astype(F64)
    s = spec_segments(o, d, nf[:, 0] - 1e-4, nf[:, 1] + 1e-4, h["dims"], r["dist"])
    sk = r["skipped"]
    assert int(sk.sum()) == r["ctr"]["n_tier_rays_untraced"]
    # soundness: no sample of a skipped ray lies in a marked voxel -- nor, deeper than DEEP voxels, in a face neighbour of one:
    # k_tier_rays refuses every voxel it walks with a distance byte <= 1, and a sample that deep inside a voxel is walked (the
    # walk's fp32 crossing times drift by ~1e-3 voxels over a few hundred steps, a tenth of DEEP)
    bad = sk & (s["dmin"] == 0)
    assert not bad.any(), "%s: skipped rays through marked voxels: %s" % (tag, np.nonzero(bad)[0][:5].tolist())
    bad = sk & (s["dmin_deep"] <= 1)
    assert not bad.any(), "%s: skipped rays through face neighbours of marked voxels: %s" % (tag, np.nonzero(bad)[0][:5].tolist())
    # never skipped: an empty interval (near >= far), an end clearly outside the box
    near_ge_far = nf[:, 0] >= nf[:, 1]
    bad = sk & (near_ge_far | (s["end_out"] & (s["face"] > RAY_FACE_EPS)))
    assert not bad.any(), "%s: skipped rays with near >= far or an end outside the box: %s" % (tag, np.nonzero(bad)[0][:5].tolist())
    # tightness: a ray inside the box that stays three voxels away is skipped
    left_out = ~s["empty"] & (s["face"] <= RAY_FACE_EPS)
    owed = ~near_ge_far & ~s["empty"] & s["inside"] & ~s["end_out"] & (s["dmin"] >= 3) & ~left_out
    bad = owed & ~sk
    assert not bad.any(), "%s: rays three voxels away that were traced: %s" % (tag, np.nonzero(bad)[0][:5].tolist())
    print("occupancy_spec | ray skip     %-24s rays %d, skipped %d, owed a skip %d, undecided (dmin 1..2 or outside) %d" % (
        tag, sk.size, sk.sum(), owed.sum(), int((~owed & ~(s["dmin"] == 0)).sum())))
    report("ray skip", tag, int(left_out.sum()), sk.size, RAY_CAP)
    return s, owed


@gpu
def test_ray_skip_on_the_fixture_frame(f7_render):
    c = f7_render
    s, owed = _judge_ray_skip(c, c["r"], c["rays"]["cam"], c["rays"]["dirs"], c["rays"]["nf"], c["tag"])
    assert owed.sum() > 0.05 * owed.size and c["r"]["skipped"].sum() < owed.size


def _hand_made_rays(h, marked, dist):
    """Rays the fixture's camera never casts, in voxel units first: (origin, direction, near, far, kind)."""
    dx, dy, dz = h["dims"]
    dimv = np.array(h["dims"], F64)
    rays = []
    add = lambda o, d, t0, t1, kind: rays.append((np.array(o, F64), np.array(d, F64), float(t0), float(t1), kind))
    spread = lambda idx, k: idx[:: max(1, len(idx) // k)][:k]
    dmin_x = dist.min(2).astype(int)          # [z, y]: the nearest marked voxel along every x row
    dmin_z = dist.min(0).astype(int)          # [y, x]
    for k in (1, 2, 3, 5):                    # rows that graze the marked region at k voxels, both ways, along x and along z
        for z, y in spread(np.argwhere(dmin_x == k), 12):
            add((0.5, y + 0.5, z + 0.5), (1, 0, 0), 0.0, dx - 1.0, "graze %d" % k)
            add((dx - 0.5, y + 0.5, z + 0.5), (-1, 0, 0), 0.0, dx - 1.0, "graze %d" % k)
        for y, x in spread(np.argwhere(dmin_z == k), 12):
            add((x + 0.5, y + 0.5, 0.5), (0, 0, 1), 0.0, dz - 1.0, "graze %d" % k)
    for z, x in spread(np.argwhere(dist.min(1) >= 3), 12):    # [z, x] columns along y that stay three voxels away
        add((x + 0.5, 0.5, z + 0.5), (0, 1, 0), 0.0, dy - 1.0, "axis y")
        add((x + 0.5, dy - 0.5, z + 0.5), (0, -1, 0), 0.0, dy - 1.0, "axis y")
    far3 = dmin_x >= 3                        # rows whose neighbours below stay away too: the plane of a voxel face, a voxel edge
    both = far3.copy()
    both[1:, :] &= far3[:-1, :]
    both[:, 1:] &= far3[:, :-1]
    both[1:, 1:] &= far3[:-1, :-1]
    both[0, :] = both[:, 0] = False
    for z, y in spread(np.argwhere(both), 16):
        add((0.5, float(y), z + 0.5), (1, 0, 0), 0.0, dx - 1.0, "face plane")
        add((0.5, float(y), float(z)), (1, 0, 0), 0.0, dx - 1.0, "edge line")
        add((-2.5, y + 0.5, z + 0.5), (1, 0, 0), 0.0, dx + 1.0, "starts outside")
        add((0.5, y + 0.5, z + 0.5), (1, 0, 0), 0.0, dx + 3.0, "ends outside")
        add((0.5, y + 0.5, z + 0.5), (1, 0, 0), 4.0, 4.0, "near == far")
        add((0.5, y + 0.5, z + 0.5), (1, 0, 0), 6.0, 4.0, "near > far")
    rng = np.random.RandomState(9)            # oblique rays between random points of the box, a third of them with a zero component
    for i in range(240):
        a, b = rng.rand(3) * dimv, rng.rand(3) * dimv
        if i % 3 == 0:
            b[i % 9 // 3] = a[i % 9 // 3]
        if np.linalg.norm(b - a) > 2.0:
            add(a, (b - a) / np.linalg.norm(b - a), 0.0, np.linalg.norm(b - a), "oblique")
    return rays


@gpu
def test_ray_skip_on_hand_made_rays(f7_render):
    """Axis rays (the d[a] == 0 branch), rays in the plane of a voxel face, rays that start or end outside the box, empty intervals,
    rays that graze the marked region at 1, 2 and 3 voxels, oblique rays: one camera per ray through hip.render."""
    c = f7_render
    h = c["r"]["h"]
    rays = _hand_made_rays(h, c["r"]["marked"], c["r"]["dist"])
    kinds = np.array([r[4] for r in rays])
    v = h["v"]
    dirs = np.array([r[1] / np.linalg.norm(r[1]) for r in rays])                         # unit directions in metres
    cam = h["origin"] + np.array([r[0] for r in rays]) * v
    nf = np.array([[r[2], r[3]] for r in rays]) * v
    r2 = _render(c, cam, dirs, nf, c["r"]["S"], c["cano"])
    assert np.array_equal(r2["marked"], c["marked"])
    s, owed = _judge_ray_skip(c, r2, cam, dirs, nf, c["tag"] + " hand-made")
    sk = r2["skipped"]
    for kind in np.unique(kinds):
        m = kinds == kind
        print("occupancy_spec | ray skip     %-24s %-15s rays %3d skipped %3d owed %3d" % (c["tag"], kind, m.sum(), sk[m].sum(), owed[m].sum()))
    for kind in ("graze 3", "axis y", "face plane", "edge line"):
        assert owed[kinds == kind].sum() >= 6, kind                                      # the cases are there and owe a skip
    for kind in ("graze 1", "starts outside", "ends outside", "near == far", "near > far"):
        assert (kinds == kind).sum() >= 6 and not sk[kinds == kind].any(), kind
    assert (s["dmin_deep"][kinds == "graze 1"] == 1).all() and (s["dmin"][kinds == "graze 2"] == 2).all()


def _classify_inputs(c, r, cam, dirs):
    """(marked, dist) of every sample from the decoded bitmap -- the point d z + cam in float64 from the fp32 depth -- and what moving
    the sample 1e-4 voxels along an axis does to them: (marked changes, smallest dist, largest dist)."""
    h = r["h"]
    f32 = np.float32
    p = np.asarray(dirs, f32).astype(F64)[:, None, :] * r["z"].astype(F64)[..., None] + np.asarray(cam, f32).astype(F64)[:, None, :]
    pv = (p - h["origin"]) * h["inv_v"]
    mk, dd, _ = spec_lookup(pv, h["dims"], r["marked"], r["dist"], valid=bool(h["valid"]))
    und, lo, hi = np.zeros(mk.shape, bool), dd.copy(), dd.copy()
    for a in range(3):
        for sgn in (-CLS_EPS, CLS_EPS):
            e = np.zeros(3)
            e[a] = sgn
            mk2, dd2, _ = spec_lookup(pv + e, h["dims"], r["marked"], r["dist"], valid=bool(h["valid"]))
            und |= mk2 != mk
            lo, hi = np.minimum(lo, dd2), np.maximum(hi, dd2)
    return mk, dd, und, lo, hi


@gpu
def test_classifier_and_promotion(f7_render):
    """A sample is undecided only if moving it 1e-4 voxels along an axis changes its (marked, dist) pair.  A ray with a sample whose
    `marked` is undecided is left out.  An undecided `dist` matters only for the choice of the nearest witness, and almost every ray
    has one: the first and last sample of a non-surface ray sit on the body box, which lies exactly two voxels inside the bitmap's
    box, on a voxel face.  Such a ray is NOT left out: every sample that can be the nearest under some admitted move is a candidate,
    and the kernel's row must be the restated row of one of them (a candidate the kernel did not choose restates a phase-1 sample
    where the kernel has none, so it cannot match by accident)."""
    c, r = f7_render, f7_render["r"]
    n, S = r["n"], r["S"]
    valid = r["state"] != TS_NONE
    mk, dd, und, dlo, dhi = _classify_inputs(c, r, c["rays"]["cam"], c["rays"]["dirs"])
    state, tier, wit = spec_classify(valid, mk, dd, r["conv"], r["mask"], r["sigma"])
    pend = valid & ~mk
    idx = np.arange(S)[None, :]
    big = 1 << 40
    key_lo = np.where(pend, dlo.astype(np.int64) * 65536 + idx, big)
    key_hi = np.where(pend, dhi.astype(np.int64) * 65536 + idx, big)
    cand = pend & (key_lo <= key_hi.min(-1)[:, None])
    n_cand = cand.sum(-1)
    K = 8
    out = (und & valid).any(-1) | (wit & (n_cand > K))
    match = (state == r["state"]).all(-1) & (tier == r["tier"])
    order = np.argsort(~cand, axis=-1, kind="stable")               # the candidates' indices first
    for k in range(K):
        alt = np.where(k < n_cand, order[:, k], order[:, 0])
        st_k, tier_k, _ = spec_classify(valid, mk, dd, r["conv"], r["mask"], r["sigma"], nearest=alt)
        match |= wit & (k < n_cand) & (st_k == r["state"]).all(-1) & (tier_k == r["tier"])
    report("classifier", c["tag"], int(out.sum()), n, CLS_CAP)
    print("occupancy_spec | classifier   %-24s witness rays %d, of them with 2+ candidates for the nearest witness %d (largest %d)" % (
        c["tag"], wit.sum(), (wit & (n_cand > 1)).sum(), n_cand[wit].max() if wit.any() else 0))
    ok = ~out
    bad = ok & ~match
    assert not bad.any(), "%d rays differ from the restated classifier, e.g. ray %d: state %s want %s, tier %d want %d" % (
        bad.sum(), np.nonzero(bad)[0][0], r["state"][bad][0].tolist(), state[bad][0].tolist(), r["tier"][bad][0], tier[bad][0])
    # per sample, on every ray: a marked sample is phase 1, on a surface ray every valid sample is
    sure = valid & ~und
    assert bool((r["state"][sure & mk] == TS_PHASE1).all()) and bool((r["state"][valid & r["conv"][:, None]] == TS_PHASE1).all())
    assert bool(((r["state"] == TS_PHASE2).any(-1) <= (r["tier"] == 2)).all()) and bool(((r["state"] == TS_PENDING).any(-1) <= (r["tier"] == 0)).all())
    # the counters, from the kernel's own final arrays
    ctr = r["ctr"]
    assert ctr["n_tier_rays"] == n and ctr["n_tier_rays_surface"] == int(r["conv"].sum()) == int((r["tier"] == 1).sum())
    assert ctr["n_tier_rays_promoted"] == int((r["tier"] == 2).sum()) and ctr["n_tier_rays_skipped"] == int((r["tier"] == 0).sum())
    assert ctr["n_tier_samples_p1"] == int((r["state"] == TS_PHASE1).sum()) and ctr["n_tier_samples_p2"] == int((r["state"] == TS_PHASE2).sum())
    assert int((wit & ok).sum()) <= ctr["n_tier_witnesses"] <= int((wit & ok).sum()) + int(out.sum())
    kinds = [int((r["tier"] == k).sum()) for k in (0, 1, 2)]
    print("occupancy_spec | classifier   %-24s rays certified / surface / promoted %s, witness rays %d, samples p1 %d p2 %d pending %d" % (
        c["tag"], kinds, ctr["n_tier_witnesses"], ctr["n_tier_samples_p1"], ctr["n_tier_samples_p2"], int((r["state"] == TS_PENDING).sum())))
    assert min(kinds) > 0 and ctr["n_tier_witnesses"] > 0 and ctr["n_tier_samples_p2"] > 0

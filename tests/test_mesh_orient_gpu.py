"""The kernels of csrc/meshorient.hpp (arah_mesh_orient / arah_mesh_boundary_loops / arah_mesh_fill_holes) against their tensor
specifications, bit for bit, on the meshes of tests/test_mesh_orient.py; the C entries on buffers of the test's own; and
geometry.orient_mesh / boundary_loops / fill_holes / repair_mesh on device tensors against the host path."""
import ctypes as C

import pytest
import torch

from test_mesh_orient import (ALL_MESHES, FILL_NAMES, LOOP_NAMES, ORIENT_NAMES, POLICIES, mesh, quant_of, spec_fill, spec_loops,
                              spec_orient)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5


def _same(got, want, names, what):
    for key, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, key)
        if g.dtype.is_floating_point:                                              # bits: a NaN is the NaN it was
            g, w = g.view(torch.int32), w.view(torch.int32)
        assert torch.equal(g.cpu(), w), (what, key)


@pytest.mark.parametrize("name", ALL_MESHES)
def test_orient_kernels_are_the_specification(name):
    from arah_release_amd import hip
    verts, faces = mesh(name)
    v, f = verts.to(DEV), faces.to(DEV)
    adj = hip.mesh_adjacency(f, verts.shape[0])
    for policy in POLICIES:
        want = spec_orient(name, policy)
        first = hip.mesh_orient(v, f, policy=policy)
        _same(first, want, ORIENT_NAMES, (name, policy))
        for again in (hip.mesh_orient(v, f.to(torch.int32), policy=policy, adjacency=adj),
                      hip.mesh_orient(v, f, policy=policy, quant=quant_of(name)[0])):
            for key, a, b in zip(ORIENT_NAMES, first, again):                      # three calls, equal bits
                assert torch.equal(a, b), (name, policy, key)
    for policy in ("seed", "majority"):                                            # the vertex count is enough for these two
        _same(hip.mesh_orient(verts.shape[0], f, policy=policy), spec_orient(name, policy), ORIENT_NAMES, (name, policy, "count"))


@pytest.mark.parametrize("name", ALL_MESHES)
def test_loop_and_fill_kernels_are_the_specification(name):
    from arah_release_amd import hip
    verts, faces = mesh(name)
    V = verts.shape[0]
    v, f = verts.to(DEV), faces.to(DEV)
    loops = hip.mesh_boundary_loops(f, V)
    _same(loops, spec_loops(name), LOOP_NAMES, name)
    adj = hip.mesh_adjacency(f, V)
    for again in (hip.mesh_boundary_loops(f.to(torch.int32), V, adjacency=adj), hip.mesh_boundary_loops(f, V)):
        for key, a, b in zip(LOOP_NAMES, loops, again):
            assert torch.equal(a, b), (name, key)
    for max_edges in (64, 5):
        want = spec_fill(name, max_edges)
        first = hip.mesh_fill_holes(v, f, max_edges=max_edges)
        _same(first, want, FILL_NAMES, (name, max_edges))                          # verts_out too: one exact rule
        for again in (hip.mesh_fill_holes(v, f.to(torch.int32), max_edges=max_edges, adjacency=adj, quant=quant_of(name)[1]),
                      hip.mesh_fill_holes(v, f, max_edges=max_edges, loops=loops)):
            for key, a, b in zip(FILL_NAMES, first, again):
                a, b = (a.view(torch.int32), b.view(torch.int32)) if a.dtype.is_floating_point else (a, b)
                assert torch.equal(a, b), (name, max_edges, key)


# ---- the C entries on the test's own buffers -----------------------------------------------------------------------------------------
def _buffers(shapes_dtypes):
    """Buffers PAD rows longer than the entry's arrays, pre-filled with a sentinel: -> (the buffers, the arrays, the paddings)."""
    bufs, arrays, pads = [], [], []
    for shape, dtype in shapes_dtypes:
        b = torch.full((shape[0] + PAD,) + tuple(shape[1:]), SENTINEL, dtype=dtype, device=DEV)
        bufs.append(b)
        arrays.append(b[:shape[0]])
        pads.append(b[shape[0]:])
    return bufs, arrays, pads


def raw_orient(verts, faces, policy, quant):
    from arah_release_amd import hip, meshing
    lib = hip.load_library()
    V, F = verts.shape[0], faces.shape[0]
    v, f = verts.to(DEV).contiguous(), faces.to(DEV).to(torch.int32).contiguous()
    adj = hip.mesh_adjacency(f, V)
    i32, i64 = torch.int32, torch.int64
    bufs, arrays, pads = _buffers([((F,), torch.uint8), ((F,), i32), ((F, 3), i32), ((F,), i32), ((F,), i32), ((F,), i64), ((F,), i64),
                                   ((6,), i32)])
    origin, scale = quant
    with hip._on_device(f.device):
        scratch = hip._mesh_cc_buf(f.device, int(lib.arah_mesh_orient_scratch_bytes(V, F)))
        rc = lib.arah_mesh_orient(hip._ptr(v), C.c_int64(V), hip._ptr(f), C.c_int64(F), *[hip._ptr(t) for t in adj[:6]],
                                  C.c_int32(meshing.ORIENT_POLICIES[policy]), (C.c_float * 3)(*origin), C.c_double(scale),
                                  *[hip._ptr(b) for b in bufs], hip._ptr(scratch), C.c_size_t(scratch.numel()), hip._stream())
    assert rc == 0
    return arrays, pads


def raw_loops_and_fill(verts, faces, max_edges, quant):
    from arah_release_amd import hip
    lib = hip.load_library()
    V, F = verts.shape[0], faces.shape[0]
    v, f = verts.to(DEV).contiguous(), faces.to(DEV).to(torch.int32).contiguous()
    adj = hip.mesh_adjacency(f, V)
    i32 = torch.int32
    lbufs, loops, lpads = _buffers([((3 * F, 2), i32), ((3 * F,), i32), ((3 * F,), i32), ((V,), i32), ((V,), torch.uint8), ((V,), i32),
                                    ((3,), i32)])
    fbufs, fill, fpads = _buffers([((V + V // 3, 3), torch.float32), ((V + V // 3,), i32), ((4 * F, 3), i32), ((4 * F,), i32), ((5,), i32)])
    origin, scale = quant
    with hip._on_device(f.device):
        scratch = hip._mesh_cc_buf(f.device, int(lib.arah_mesh_boundary_loops_scratch_bytes(V, F)))
        rc = lib.arah_mesh_boundary_loops(hip._ptr(f), C.c_int64(F), C.c_int64(V), *[hip._ptr(t) for t in adj[2:6]],
                                          *[hip._ptr(b) for b in lbufs], hip._ptr(scratch), C.c_size_t(scratch.numel()), hip._stream())
        assert rc == 0
        scratch = hip._mesh_cc_buf(f.device, int(lib.arah_mesh_fill_holes_scratch_bytes(V, F)))
        e, _, el, le, ls, lv, lc = lbufs
        rc = lib.arah_mesh_fill_holes(hip._ptr(v), C.c_int64(V), hip._ptr(f), C.c_int64(F), hip._ptr(e), hip._ptr(el), hip._ptr(le),
                                      hip._ptr(ls), hip._ptr(lv), hip._ptr(lc), C.c_int32(max_edges), (C.c_float * 3)(*origin),
                                      C.c_double(scale), *[hip._ptr(b) for b in fbufs], hip._ptr(scratch), C.c_size_t(scratch.numel()),
                                      hip._stream())
        assert rc == 0
    return loops, lpads, fill, fpads


@pytest.mark.parametrize("name", ["empty", "no_faces", "one_tri", "bad_faces", "moebius16", "noise20_r", "sphere33_hr", "sphere33_touch"])
def test_c_entries_on_the_tests_own_buffers(name):
    """Rows beyond the arrays come back untouched; rows beyond the counts, inside the arrays, zero as the specification has them."""
    verts, faces = mesh(name)
    for policy in ("majority", "negative"):
        arrays, pads = raw_orient(verts, faces, policy, quant_of(name)[0])
        _same(arrays, spec_orient(name, policy), ORIENT_NAMES, (name, policy))
        assert all(bool((p == SENTINEL).all()) for p in pads), (name, policy)
    loops, lpads, fill, fpads = raw_loops_and_fill(verts, faces, 64, quant_of(name)[1])
    _same(loops, spec_loops(name), LOOP_NAMES, name)
    _same(fill, spec_fill(name, 64), FILL_NAMES, name)
    assert all(bool((p == SENTINEL).all()) for p in lpads + fpads), name


def _open_strip(n_faces):
    """A consistently oriented open triangle strip: F faces over F + 2 vertices, whose boundary is one simple loop of F + 2 half-edges."""
    i = torch.arange(n_faces)
    odd = i % 2 == 1
    faces = torch.stack([torch.where(odd, i + 1, i), torch.where(odd, i, i + 1), i + 2], 1)
    k = torch.arange(n_faces + 2)
    return torch.stack([0.25 * (k // 2), 1.0 * (k % 2), 0.125 * (k % 3)], 1).float(), faces


def _disjoint_triangles(n):
    """n triangles that share nothing: 3 n vertices, n simple loops of 3 half-edges each."""
    k = torch.arange(n).float()[:, None, None]
    corner = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.0, 0.25], [0.0, 0.75, 0.125]])
    return (corner[None] + k * torch.tensor([1.0, 0.0, 0.0])).reshape(3 * n, 3), torch.arange(3 * n).reshape(n, 3)


# The three instances of k_mo_compact on either side of a chunk of 1024 elements, which the named meshes never reach.  Strips: the
# boundary walk covers 3 F = 1023, 1026, 2049 (face, corner) pairs.  Disjoint triangles: the loop walk covers 3 n slots and is cut
# at the n loops the device counted, the filled-edge walk covers 3 n boundary edges.
@pytest.mark.parametrize("family, n, max_edges", [("strip", 341, 4096), ("strip", 342, 4096), ("strip", 683, 4096),
                                                   ("triangles", 1024, 3), ("triangles", 1025, 3)])
def test_compaction_walks_on_either_side_of_a_chunk(family, n, max_edges):
    from arah_release_amd import meshing
    verts, faces = _open_strip(n) if family == "strip" else _disjoint_triangles(n)
    V, F = verts.shape[0], faces.shape[0]
    want_loops = meshing.mesh_boundary_loops(faces, V)
    want_fill = meshing.mesh_fill_holes(verts, faces, max_edges=max_edges)
    if family == "strip":                                                          # one loop round the strip, closed by one fan
        assert want_loops[-1].tolist() == [n + 2, 1, 1] and want_fill[-1].tolist() == [n + 2, 1, 1, 1, n + 2]
    else:                                                                          # n loops, n added vertices, 3 n added faces
        assert (V, V // 3) == (3 * n, n) and want_loops[-1].tolist() == [3 * n, n, n] and want_fill[-1].tolist() == [3 * n, n, n, n, 3 * n]
        assert want_fill[1][V:].tolist() == list(range(0, V, 3)) and bool((want_fill[3][F:] == torch.arange(n).repeat_interleave(3)).all())
    loops, lpads, fill, fpads = raw_loops_and_fill(verts, faces, max_edges, meshing.fill_quant(verts))
    _same(loops, want_loops, LOOP_NAMES, (family, n))
    _same(fill, want_fill, FILL_NAMES, (family, n))
    assert all(bool((p == SENTINEL).all()) for p in lpads + fpads), (family, n)


def test_faces_without_vertices_and_vertices_without_faces():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("sphere17_r")
    none = torch.zeros(0, 3)
    for v, f in ((none, faces), (verts, faces[:0]), (none, faces[:0])):            # V = 0: every face is invalid
        for policy in POLICIES:
            _same(hip.mesh_orient(v.to(DEV), f.to(DEV), policy=policy), meshing.mesh_orient(v, f, policy=policy), ORIENT_NAMES, policy)
        _same(hip.mesh_boundary_loops(f.to(DEV), v.shape[0]), meshing.mesh_boundary_loops(f, v.shape[0]), LOOP_NAMES, "loops")
        _same(hip.mesh_fill_holes(v.to(DEV), f.to(DEV)), meshing.mesh_fill_holes(v, f), FILL_NAMES, "fill")
        arrays, pads = raw_orient(v, f, "positive", ([0.0, 0.0, 0.0], 1.0))
        _same(arrays, meshing.mesh_orient(v, f, policy="positive"), ORIENT_NAMES, "raw")
        loops, lpads, fill, fpads = raw_loops_and_fill(v, f, 64, ([0.0, 0.0, 0.0], 1.0))
        _same(loops, meshing.mesh_boundary_loops(f, v.shape[0]), LOOP_NAMES, "raw loops")
        _same(fill, meshing.mesh_fill_holes(v, f), FILL_NAMES, "raw fill")
        assert all(bool((p == SENTINEL).all()) for p in pads + lpads + fpads)


def test_entries_validate():
    from arah_release_amd import hip
    verts, faces = mesh("sphere17_r")
    V, F = verts.shape[0], faces.shape[0]
    v, f = verts.to(DEV), faces.to(DEV)
    adj = hip.mesh_adjacency(f, V)
    for bad in (lambda: hip.mesh_orient(verts, f), lambda: hip.mesh_orient(v, faces), lambda: hip.mesh_orient(v.double(), f),
                lambda: hip.mesh_orient(V, f, policy="negative"), lambda: hip.mesh_orient(v, f, policy="largest"),
                lambda: hip.mesh_orient(v, f, adjacency=adj[:5]), lambda: hip.mesh_orient(v, f, adjacency=tuple(t.cpu() for t in adj)),
                lambda: hip.mesh_orient(v, f, policy="negative", quant=([0.0, 0.0, float("nan")], 1.0)),
                lambda: hip.mesh_orient(v, f, policy="negative", quant=([0.0, 0.0, 0.0], 0.0)),
                lambda: hip.mesh_boundary_loops(faces, V), lambda: hip.mesh_boundary_loops(f, -1),
                lambda: hip.mesh_fill_holes(v, f, max_edges=-1), lambda: hip.mesh_fill_holes(v, f, max_edges=2 ** 26 + 1),
                lambda: hip.mesh_fill_holes(v, f, loops=hip.mesh_boundary_loops(f, V)[:6]),
                lambda: hip.mesh_fill_holes(v[:-1], f, loops=hip.mesh_boundary_loops(f, V))):
        with pytest.raises(ValueError):
            bad()
    lib = hip.load_library()
    BADARG, WORKSPACE = -1, -3
    p, i32, i64 = hip._ptr, torch.int32, torch.int64
    f32 = f.to(i32).contiguous()
    out = hip.mesh_orient(v, f32, policy="negative")
    kept = [t.clone() for t in out]
    need = int(lib.arah_mesh_orient_scratch_bytes(V, F))
    scratch = torch.empty(need, dtype=torch.uint8, device=DEV)

    def orient(policy=2, scale=1.0, n_faces=F, n_verts=V, verts_p=p(v), missing=None, nbytes=need):
        outs = [None if i == missing else p(t) for i, t in enumerate(out)]
        return lib.arah_mesh_orient(verts_p, C.c_int64(n_verts), p(f32), C.c_int64(n_faces), *[p(t) for t in adj[:6]], C.c_int32(policy),
                                    (C.c_float * 3)(0.0, 0.0, 0.0), C.c_double(scale), *outs, p(scratch), C.c_size_t(nbytes),
                                    hip._stream(DEV))
    assert orient(policy=4) == BADARG and orient(policy=-1) == BADARG and orient(scale=0.0) == BADARG
    assert orient(scale=float("inf")) == BADARG and orient(verts_p=None) == BADARG
    assert orient(n_faces=-1) == BADARG and orient(n_faces=2 ** 28 + 1) == BADARG and orient(n_verts=2 ** 31) == BADARG
    for missing in range(8):
        assert orient(missing=missing) == BADARG, ORIENT_NAMES[missing]
    assert orient(nbytes=need - 1) == WORKSPACE
    torch.cuda.synchronize()
    for a, b in zip(out, kept):                                                    # the refused calls launched nothing
        assert torch.equal(a, b)
    for query in (lib.arah_mesh_orient_scratch_bytes, lib.arah_mesh_boundary_loops_scratch_bytes, lib.arah_mesh_fill_holes_scratch_bytes):
        assert query(0, 0) > 0 and query(2 ** 31 - 1, 2 ** 28) > query(1000, 1000) > 0
        assert query(-1, 0) == 0 and query(0, -1) == 0 and query(2 ** 31, 0) == 0 and query(0, 2 ** 28 + 1) == 0


# ---- through geometry.* on device tensors ------------------------------------------------------------------------------------------------
def _same_dict(got, want, what):
    assert set(got) == set(want), what
    for key, w in want.items():
        g = got[key]
        if isinstance(w, torch.Tensor):
            assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w), (what, key)
        elif isinstance(w, dict):
            _same_dict(g, w, (what, key))
        else:
            assert g == w, (what, key)


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_public_entries_on_the_device_are_the_host_path(dtype):
    from arah_release_amd import geometry
    for name in ("sphere33_hr", "noise20_r", "bad_faces", "moebius16", "empty"):
        verts, faces = mesh(name)
        faces = faces.to(dtype)
        v, f = verts.to(DEV), faces.to(DEV)
        for policy in POLICIES:
            _same_dict(geometry.orient_mesh(v, f, policy=policy), geometry.orient_mesh(verts, faces, policy=policy), (name, policy))
        _same_dict(geometry.boundary_loops(v, f), geometry.boundary_loops(verts, faces), name)
        colour = torch.rand(verts.shape[0], 3, generator=torch.Generator().manual_seed(4))
        got = geometry.fill_holes(v, f, max_edges=6, attributes={"colour": colour.to(DEV)}, adjacency=geometry.mesh_adjacency(v, f))
        want = geometry.fill_holes(verts, faces, max_edges=6, attributes={"colour": colour})
        assert got["faces"].dtype == dtype
        _same_dict(got, want, name)
    verts, faces = mesh("sphere33_hr")
    got = geometry.repair_mesh(verts.to(DEV), faces.to(dtype).to(DEV))
    want = geometry.repair_mesh(verts, faces.to(dtype))
    assert got["topology"]["watertight"] and got["faces"].dtype == dtype
    _same_dict(got, want, "repair")


def test_normals_and_winding_numbers_of_the_oriented_mesh_are_the_originals():
    from arah_release_amd import geometry
    verts, original = mesh("sphere17")
    _, reversed_faces = mesh("sphere17_r")
    v = verts.to(DEV)
    wrong = geometry.vertex_normals(v, reversed_faces.to(DEV))
    want = geometry.vertex_normals(v, original.to(DEV))
    assert not torch.equal(wrong, want)                                            # a reversed patch cancels its neighbours
    oriented = geometry.orient_mesh(v, reversed_faces.to(DEV), policy="negative")["faces"]
    assert torch.equal(oriented.cpu(), original)
    assert torch.equal(geometry.vertex_normals(v, oriented).view(torch.int32), want.view(torch.int32))
    points = (torch.rand(200, 3, generator=torch.Generator().manual_seed(6)) * 2.0 - 1.0).to(DEV)
    w_closed = geometry.winding_number((v, original.to(DEV)), points)
    w_oriented = geometry.winding_number((v, oriented), points)
    assert w_closed.dtype == torch.float64 and torch.equal(w_oriented, w_closed)
    assert not torch.equal(geometry.winding_number((v, reversed_faces.to(DEV)), points), w_closed)

"""The kernels of csrc/meshflip.hpp (arah_mesh_flip_round) against their tensor specification meshing.mesh_flip_round, bit for bit
in every output and counter, on the meshes of tests/test_mesh_flip.py, round after round until no candidate is left; empty inputs;
the C entry on buffers of the test's own; geometry.flip_edges on device tensors against the same call on the host."""
import ctypes as C

import pytest
import torch

from test_mesh_flip import CRITERIA, counts_of, mesh, same_bits, spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A
PAD = 5
SMALL = ("tetrahedron", "octahedron", "flat_bipyramid", "kite", "sheet", "three_faces", "misoriented", "nan_vertex", "bad_ids",
         "open_sphere", "bicone40")


def run(name, criterion, salt, faces_dtype=torch.int32):
    from arah_release_amd import hip
    verts, faces = mesh(name)
    return hip.mesh_flip_round(verts.to(DEV), faces.to(DEV).to(faces_dtype), criterion, salt, details=True)


@pytest.mark.parametrize("name", SMALL)
def test_kernels_are_the_specification(name):
    for criterion, salt in (("delaunay", 0), ("valence", 0), ("delaunay", 2 ** 32 - 1), ("valence", 5)):
        want = spec(name, criterion, salt)
        first = run(name, criterion, salt)
        same_bits(first, want, (name, criterion, salt), n=5)
        # again, from faces of another integer type: the order of arrival in the adjacency build and in the locks does not show
        same_bits(run(name, criterion, salt, faces_dtype=torch.int64), first, (name, criterion, salt, "again"))


# jgrid33: 2 048 faces and 6 272 = 98 x 64 neighbour entries, whole waves; jgrid9: 416 entries, six waves and a half; sphere33 and
# f10: 5 k faces and 31 k entries, several workgroups of every launch
@pytest.mark.parametrize("name", ["jgrid9_0", "jgrid33_1", "sphere33", "f10"])
@pytest.mark.parametrize("criterion", CRITERIA)
def test_rounds_on_the_device_are_the_specification_until_none_is_left(name, criterion):
    from arah_release_amd import geometry, hip, meshing
    verts, faces = mesh(name)
    entries = int(meshing.mesh_adjacency(faces, verts.shape[0])[2][-1])
    assert (entries % 64 == 0) == (name == "jgrid33_1") and (name == "jgrid9_0" or faces.shape[0] >= 2048)
    dv, f, df = verts.to(DEV), faces, faces.to(DEV).to(torch.int32)
    history = []
    for salt in range(64):
        want = meshing.mesh_flip_round(verts, f, criterion, salt, details=True)
        got = hip.mesh_flip_round(dv, df, criterion, salt, details=True)
        same_bits(got, want, (name, criterion, "round", salt), n=5)
        c = counts_of(want)
        history.append(c["candidates"])
        if c["candidates"] == 0:
            break
        f, df = want[0].long(), got[0]
    assert history[-1] == 0 and (len(history) > 3 or (name.startswith("jgrid") and criterion == "valence"))
    ref = geometry.flip_edges(verts, faces, criterion)
    res = geometry.flip_edges(dv, faces.to(DEV), criterion)
    assert res["faces"].is_cuda and res["faces"].dtype == faces.dtype and torch.equal(res["faces"].cpu(), ref["faces"])
    assert {k: x for k, x in res.items() if k != "faces"} == {k: x for k, x in ref.items() if k != "faces"}
    assert res["candidates"] == history and res["converged"] and torch.equal(ref["faces"], f)


def test_empty_meshes_write_their_counts():
    from arah_release_amd import hip, meshing
    verts, faces = mesh("octahedron")
    dv, df = verts.to(DEV), faces.to(DEV)
    for v, f, hv, hf in ((dv[:0], df[:0], verts[:0], faces[:0]), (dv, df[:0], verts, faces[:0]), (dv[:0], df, verts[:0], faces)):
        for criterion in CRITERIA:
            same_bits(hip.mesh_flip_round(v, f, criterion, 1, details=True), meshing.mesh_flip_round(hv, hf, criterion, 1, details=True),
                      (v.shape, f.shape, criterion), n=5)


def test_entry_writes_its_arrays_and_nothing_else():
    from arah_release_amd import hip
    name = "bad_ids"
    verts, faces = mesh(name)
    want = spec(name, "delaunay", 3)
    verts, f32 = verts.to(DEV), faces.to(DEV).to(torch.int32).contiguous()
    lib = hip.load_library()
    V, F = verts.shape[0], f32.shape[0]

    def buf(nbytes):
        return torch.full((nbytes + PAD,), SENTINEL, dtype=torch.uint8, device=DEV)
    sizes = (F * 12, F, 9 * 4, 6 * F * 8, 6 * F)                                  # faces_out, face_flag, counts, edge_key, edge_reason
    need = int(lib.arah_mesh_flip_round_scratch_bytes(V, F))
    with hip._on_device(verts.device):
        scratch = buf(need)                                                       # the test's own, padded like the outputs
        for nbytes, crit, rc_want in ((need - 1, 0, -3), (need, 2, -1), (need, 0, 0)):   # the refused calls launch nothing
            bufs = [buf(n) for n in sizes]
            rc = lib.arah_mesh_flip_round(hip._ptr(verts), C.c_int64(V), hip._ptr(f32), C.c_int64(F), C.c_int32(crit), C.c_uint32(3),
                                          *[hip._ptr(b) for b in bufs], hip._ptr(scratch), C.c_size_t(nbytes), hip._stream())
            torch.cuda.synchronize()
            assert rc == rc_want
            if rc:
                assert all(bool((b == SENTINEL).all()) for b in bufs) and bool((scratch == SENTINEL).all())
    for b, n in zip(bufs + [scratch], sizes + (need,)):
        assert bool((b[n:] == SENTINEL).all())
    kinds = (torch.int32, torch.uint8, torch.int32, torch.int64, torch.uint8)
    shapes = ((F, 3), (F,), (9,), (6 * F,), (6 * F,))
    got = [b[:n].view(k).reshape(s) for b, n, k, s in zip(bufs, sizes, kinds, shapes)]
    same_bits(got, want, "raw entry", n=5)
    c = counts_of(want)
    assert 0 < c["selected"] < c["candidates"] < c["edges"] and torch.equal(got[0][100:104].cpu().long(), faces[100:104])

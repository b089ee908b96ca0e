// mcubes.hpp -- marching cubes of the canonical-mesh branch on the device, without a host round trip.
//
// Reference: utils/sdf_meshing.py:83-101 hands the 256^3 SDF volume to skimage.measure.marching_cubes_lewiner on the CPU
// (models/__init__.py:203-311 then skins and rasterises the mesh).  Round 2-4 of this build ran the same extraction as ~30
// torch operations over the surface cells (meshing.marching_cubes: torch.nonzero / repeat_interleave, i.e. two device -> host
// round trips per frame, a 256^3 int64 case volume); this is that function as three kernels, triangle for triangle:
//
//   k_mcubes<kMcCount>  one workgroup per lattice row (ix, iy), one thread per cell iz: the 8 corner values, the inside / outside
//                    pattern, the triangle count of the case -> triangles per row
//   k_mc_scan        exclusive scan of the row counts (one workgroup, meshcommon.hpp) -> first triangle of every row, the total
//   k_mcubes<kMcSoup>  the same walk again; a cell writes its triangles at row base + prefix inside the row
//   k_mc_pad         zero-fills the unused tail of the caller's buffer: triangles beyond the count are degenerate (all
//                    three corners equal), which every later stage -- skinning, projection, rasterisation -- ignores
//
// Output ORDER is the torch formulation's: cells in (ix, iy, iz) order, a cell's triangles in table order; the crossing
// point of a lattice edge is interpolated from its lower to its higher end whichever cell asks (shared vertices are
// bit-equal: the mesh is watertight), every operation rounded on its own like the tensor expression
// (pa + t (pb - pa)) * vs - 1 (no fma contraction); orientation: right-hand normals down the gradient.
// The case table (which edges of a cell form its triangles) is the CALLER's: a device copy of meshing.case_table().
// The same level set as an INDEXED mesh (shared vertices, faces of vertex ids): the second half of this file.
#pragma once

constexpr int kMcTableWidth = 16;   // 5 triangles x 3 edge ids, padded

__device__ __constant__ signed char kMcCorner[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}, {0, 1, 1}};
__device__ __constant__ signed char kMcEdge[12][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {4, 5}, {5, 6}, {6, 7}, {7, 4}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};

// Crossing point of the lattice edge that leaves point p along `axis`, from its LOWER end (value sa) to its higher end (sb):
// the tensor expression (pa + t (pb - pa)) * vs - 1 with one rounding per operation (hipcc contracts * and + into fma by
// default, and __fmul_rn / __fadd_rn are plain operators to it).  The soup's corners and the indexed mesh's vertices both come
// from here, so a vertex is bit-equal to every soup corner on its edge.
__device__ __forceinline__ void mc_edge_point(float sa, float sb, float level, float vs, const int p[3], int axis, float out[3]) {
#pragma clang fp contract(off)
    const float va = sa - level;
    const float vb = sb - level;
    const float t = fminf(fmaxf(va / (va - vb), 0.0f), 1.0f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float d = c == axis ? 1.0f : 0.0f;
        out[c] = ((float)p[c] + t * d) * vs - 1.0f;
    }
}

// Orientation of a triangle v of a cell with corner values cv: right-hand normals point DOWN the gradient of the corner
// values; true = corners 1 and 2 change places.
__device__ __forceinline__ bool mc_flip(const float v[3][3], const float cv[8]) {
#pragma clang fp contract(off)
    float grad[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) grad[k] = grad[k] + (kMcCorner[c][k] ? cv[c] : -cv[c]);
    float e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        e1[c] = v[1][c] - v[0][c];
        e2[c] = v[2][c] - v[0][c];
    }
    const float nx = e1[1] * e2[2] - e1[2] * e2[1];
    const float ny = e1[2] * e2[0] - e1[0] * e2[2];
    const float nz = e1[0] * e2[1] - e1[1] * e2[0];
    const float dn = (nx * grad[0] + ny * grad[1]) + nz * grad[2];
    return dn > 0.f;
}

// Crossing flags of the lattice edges that leave point (ix, iy, iz) upwards along the axes below n_axes: bit a set = the edge
// along axis a exists (the point is not on that axis' last layer) and its two ends lie on different sides of the level.
__device__ __forceinline__ int mc_point_flags(const float* __restrict__ sdf, int N, float level, int ix, int iy, int iz, int n_axes) {
    const size_t p = ((size_t)ix * N + iy) * N + iz;
    const bool in0 = sdf[p] < level;
    int flags = 0;
    if (n_axes > 0 && ix + 1 < N && (sdf[p + (size_t)N * N] < level) != in0) flags |= 1;
    if (n_axes > 1 && iy + 1 < N && (sdf[p + N] < level) != in0) flags |= 2;
    if (n_axes > 2 && iz + 1 < N && (sdf[p + 1] < level) != in0) flags |= 4;
    return flags;
}

enum { kMcCount = 0, kMcSoup = 1, kMcFaces = 2 };

// MODE kMcCount: triangles per row -> row_count.  kMcSoup: the triangles -> tris [cap][3][3].  kMcFaces: the same triangles as
// vertex ids of the indexed mesh -> faces [cap][3]; first_vert [N^3] is the id of every lattice point's first vertex.
template <int MODE>
__global__ __launch_bounds__(kImeshThreads) void k_mcubes(const float* __restrict__ sdf, int N, float level, float vs,
                                                          const signed char* __restrict__ table, const int* __restrict__ ntri,
                                                          int* __restrict__ row_count, const int* __restrict__ row_base,
                                                          float* __restrict__ tris, int cap,
                                                          const int* __restrict__ first_vert, int* __restrict__ faces) {
    constexpr bool EMIT = MODE != kMcCount;
    __shared__ int wsum[kImeshThreads / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x, M = N - 1;
    const int ix = row / M, iy = row - ix * M;
    int done = 0;   // triangles of this row in front of the current chunk of cells
    for (int z0 = 0; z0 < M; z0 += kImeshThreads) {
        const int iz = z0 + tid;
        const bool ok = iz < M;
        float cv[8];
        int cs = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            cv[c] = ok ? sdf[((size_t)(ix + kMcCorner[c][0]) * N + (iy + kMcCorner[c][1])) * N + (iz + kMcCorner[c][2])] : 0.f;
            cs |= (cv[c] < level ? 1 : 0) << c;
        }
        const int cnt = (ok && cs != 0 && cs != 255) ? ntri[cs] : 0;
        int total;
        const int before = mesh_prefix(cnt, wsum, total);   // the triangles of the chunk's cells below this one
        if constexpr (EMIT) {
            const int first = row_base[row] + done + before;
            for (int s = 0; s < cnt; ++s) {
                if (first + s >= cap) break;
                float v[3][3];
                int id[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int e = table[cs * kMcTableWidth + 3 * s + k];
                    int a = kMcEdge[e][0], b = kMcEdge[e][1];
                    // from the lower to the higher end of the lattice edge (the two ends differ in one coordinate)
                    if (kMcCorner[a][0] > kMcCorner[b][0] || kMcCorner[a][1] > kMcCorner[b][1] || kMcCorner[a][2] > kMcCorner[b][2]) {
                        const int t = a;
                        a = b;
                        b = t;
                    }
                    const int axis = kMcCorner[b][0] != kMcCorner[a][0] ? 0 : (kMcCorner[b][1] != kMcCorner[a][1] ? 1 : 2);
                    // the two end values are read again rather than taken from cv[]: a and b are run-time indices, and a
                    // register array indexed at run time lives in scratch
                    const int pa[3] = {ix + kMcCorner[a][0], iy + kMcCorner[a][1], iz + kMcCorner[a][2]};
                    const int pb[3] = {ix + kMcCorner[b][0], iy + kMcCorner[b][1], iz + kMcCorner[b][2]};
                    const size_t la = ((size_t)pa[0] * N + pa[1]) * N + pa[2];
                    mc_edge_point(sdf[la], sdf[((size_t)pb[0] * N + pb[1]) * N + pb[2]], level, vs, pa, axis, v[k]);
                    if constexpr (MODE == kMcFaces)
                        id[k] = first_vert[la] + __popc(mc_point_flags(sdf, N, level, pa[0], pa[1], pa[2], axis));
                }
                const bool flip = mc_flip(v, cv);
                if constexpr (MODE == kMcSoup) {
                    float* o = tris + (size_t)(first + s) * 9;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        o[c] = v[0][c];
                        o[3 + c] = flip ? v[2][c] : v[1][c];
                        o[6 + c] = flip ? v[1][c] : v[2][c];
                    }
                } else {
                    int* o = faces + (size_t)(first + s) * 3;
                    o[0] = id[0];
                    o[1] = flip ? id[2] : id[1];
                    o[2] = flip ? id[1] : id[2];
                }
            }
        }
        done += total;
    }
    if (MODE == kMcCount && tid == 0) row_count[row] = done;
}

__global__ void k_mc_pad(float* __restrict__ tris, const int* total, int cap) {
    const size_t first = (size_t)min(max(*total, 0), cap) * 9, end = (size_t)cap * 9;
    for (size_t i = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += (size_t)gridDim.x * blockDim.x) tris[i] = 0.f;
}

// ---- indexed mesh: one vertex per crossing lattice edge ------------------------------------------------------------------
// A marching-cubes vertex lies on a lattice edge, and a lattice edge has an integer name: its lower end (ix, iy, iz) and its
// axis a, key ((ix N + iy) N + iz) 3 + a.  The vertices are the crossing edges in ascending key order, numbered by the same
// count / scan / fill as the triangles (meshcommon.hpp: mesh_prefix inside a row, k_mc_scan over the rows, k_mc_pad_words):
//
//   k_mc_verts<false>  one workgroup per lattice row (ix, iy), one thread per POINT iz: its up to three crossing flags
//                      (mc_point_flags) -> vertices per row
//   k_mc_scan          first vertex of every row, the total
//   k_mc_verts<true>   the same walk; a point writes the id of its first vertex to first_vert [N^3] and its vertices
//                      (mc_edge_point: bit-equal to the soup's corners) and keys at row base + prefix inside the row
//   k_mcubes<kMcCount>, k_mc_scan, k_mcubes<kMcFaces>   the soup's cell walk; a corner on the edge (p, a) is vertex
//                      first_vert[p] + popcount(flags(p) below a), the orientation flip is the soup's own (mc_flip)
//   k_mc_pad_words     zero-fills the rows between the counts and the caps
//
// No hashing, no sorting, no atomics: the result is deterministic.
template <bool EMIT>
__global__ __launch_bounds__(kImeshThreads) void k_mc_verts(const float* __restrict__ sdf, int N, float level, float vs,
                                                            int* __restrict__ row_count, const int* __restrict__ row_base,
                                                            int* __restrict__ first_vert, float* __restrict__ verts,
                                                            int* __restrict__ vert_edge, int cap) {
    __shared__ int wsum[kImeshThreads / 64];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const int ix = row / N, iy = row - ix * N;
    int done = 0;   // vertices of this row in front of the current chunk of points
    for (int z0 = 0; z0 < N; z0 += kImeshThreads) {
        const int iz = z0 + tid;
        const bool ok = iz < N;
        const int flags = ok ? mc_point_flags(sdf, N, level, ix, iy, iz, 3) : 0;
        const int cnt = __popc(flags);
        int total;
        const int before = mesh_prefix(cnt, wsum, total);   // the vertices of the chunk's points below this one
        if constexpr (EMIT) {
            if (ok) {
                const size_t p = ((size_t)row * N) + iz;
                int id = row_base[row] + done + before;
                first_vert[p] = id;
                const int pp[3] = {ix, iy, iz};
                const size_t step[3] = {(size_t)N * N, (size_t)N, 1};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (!(flags & (1 << a))) continue;
                    if (id < cap) {
                        float v[3];
                        mc_edge_point(sdf[p], sdf[p + step[a]], level, vs, pp, a, v);
                        verts[(size_t)id * 3 + 0] = v[0];
                        verts[(size_t)id * 3 + 1] = v[1];
                        verts[(size_t)id * 3 + 2] = v[2];
                        if (vert_edge) vert_edge[id] = (int)p * 3 + a;
                    }
                    ++id;
                }
            }
        }
        done += total;
    }
    if (!EMIT && tid == 0) row_count[row] = done;
}

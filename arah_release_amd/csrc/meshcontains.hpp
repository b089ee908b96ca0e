// meshcontains.hpp -- is a point inside a mesh, for LARGE meshes: libmesh's check_mesh_contains (reference
// im2mesh/utils/libmesh/inside_mesh.py) with its TriangleHash (triangle_hash.pyx) restated on the device, occupancy grids.
//
// The rule is meshing.mesh_contains, and every result equals it bit for bit.  float64 throughout, rounded operation by operation
// (contraction off wherever the rule's arithmetic runs):
//
//   * lo / hi over the vertices some face uses; scale = (resolution - 1) / (hi - lo), translate = 0.5 - scale * lo,
//     q = scale * x + translate for points and triangle corners alike (MeshBox of meshquery.hpp);
//   * the mesh is VALID when it has a face, every face id lies in [0, V), every used vertex is finite and hi > lo on all three
//     axes; against any other mesh every point is outside, not ambiguous, and has tested 0 candidates;
//   * in_box: 0 <= q <= resolution on all three axes (a NaN makes it false);
//   * the hash is two-dimensional, over xy: a point reads the ONE cell ((int)q.x, (int)q.y) -- none when either is
//     outside [0, resolution) --, triangle t is listed in the cells [clip((int)min_t), clip((int)max_t)] of its rescaled corners on both
//     axes, clipped to [0, resolution - 1]; a triangle appears at most once in a cell, so nothing is de-duplicated;
//   * per candidate the strict 2-D test and the depth comparison of k_mesh_query (meshquery.hpp:151-171), ct_test2d below;
//   * inside = in_box & n0 odd & n1 odd, ambiguous = in_box & (parity of n0 != parity of n1).
//
// The index, one launch per line (arah_contains_index_count):
//
//   k_ct_box       lo / hi / validity -> header                                                  (one workgroup)
//   k_ct_setup     one lane per face: the RECORD (16 doubles: everything of the rule that depends on the triangle alone, each
//                  value by the rule's own operation sequence), the clipped cell rectangle, and the face's class by the cells n
//                  of its rectangle: lane (n <= kCtLaneCells), wave (<= kCtWaveCells), workgroup (<= kCtGroupCells: the MEDIUM
//                  list), several workgroups (the HUGE list, kCtParts parts a face)
//   k_ct_walk      lane and wave classes: +1 per cell of the rectangle (integer atomicAdd); the wave's turns are mesh_wave_turns
//   k_ct_walk_lists  the two lists (mesh_list_walk of meshcommon.hpp): one face covering all resolution^2 cells is spread over
//                  kCtParts workgroups and does not serialise the build
//   k_ct_scan_a/b/c  exclusive scan of the counts -> start[resolution^2 + 1]; the total (64-bit) goes to the header
//
// The total is data-dependent: the caller reads it from the header -- the index's ONE host synchronisation --, allocates the
// reference array, and arah_contains_index_fill runs the two walks again, now claiming slots (atomicAdd on a cursor per cell that
// starts at start[cell]).  The order of the ids inside a cell depends on the order of arrival and is never seen: the parities are
// integer sums.  Integer atomics only.  No thread waits for another; every loop ends by an argument stated at the loop.
// Included by arah_hip.hip after meshquery.hpp.
#pragma once

namespace {

constexpr int kCtThreads = 256;
constexpr int kCtMaxRes = 4096;
constexpr int kCtRec = 16;               // doubles of a triangle's record
// class thresholds, in cells of a clipped rectangle: NOT measured, chosen like meshraster.hpp's (a 256^3 marching-cubes face covers
// one to four cells at resolution 512)
constexpr int kCtLaneCells = 16;
constexpr int kCtWaveCells = 512;
constexpr int kCtGroupCells = 1 << 15;
constexpr int kCtParts = 64;
constexpr int kCtListGrid = 2048;
constexpr int kCtScanPer = 8;            // cells a thread scans
constexpr int kCtScanBlock = kCtThreads * kCtScanPer;
constexpr int kCtGridZ = 64 * 64;        // lattice points of a column one wave answers: 64 lanes x 64 parity bits

struct CtHeader {
    MeshBox box;                 // 56 bytes
    long long n_refs;            // total references (offset 56)
    int n_faces, resolution;     // offset 64, 68
    int valid;                   // offset 72
    int status;                  // offset 76: bit 0 = more than INT32_MAX references
    unsigned n_med, n_huge;      // offset 80, 84
};

struct CtIndex {
    CtHeader* hdr;
    double* rec;                 // [F][kCtRec]
    int* rect;                   // [F][4] ix0, ix1, iy0, iy1 (ix1 < ix0: no cell)
    int* med;                    // [F]
    int* huge;                   // [F]
    unsigned* cnt;               // [R^2] counts, then the fill's cursors
    unsigned* start;             // [R^2 + 1]
    unsigned long long* sums;    // [ceil(R^2 / kCtScanBlock)]
    size_t bytes;
};

struct CtRect {   // a face's clipped rectangle as the walks take it: first cell, cells per row
    int ix0, iy0, h;
};

// lo / hi over the used vertices, validity, the two list counters
__global__ __launch_bounds__(kCtThreads) void k_ct_box(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                       int n_faces, int res, CtHeader* hdr) {
    static_assert(kCtThreads == kBoxThreads, "mesh_box_reduce");
    __shared__ double smin[3][kCtThreads], smax[3][kCtThreads];
    __shared__ int sbad[kCtThreads];
    const int tid = threadIdx.x;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    int bad = 0;
    // terminates: 3 n_faces - i strictly decreases (3 n_faces <= 3 * 2^28 fits a long long)
    for (long long i = tid; i < 3ll * n_faces; i += kCtThreads) {
        const int v = faces[i];
        if ((unsigned)v >= (unsigned)n_verts) {
            bad = 1;
            continue;
        }
        for (int c = 0; c < 3; ++c) {
            const double x = (double)verts[(size_t)v * 3 + c];
            if (!isfinite(x)) bad = 1;
            lo[c] = fmin(lo[c], x);
            hi[c] = fmax(hi[c], x);
        }
    }
    mesh_box_reduce(lo, hi, bad, smin, smax, sbad, [](int) {});
    if (tid < 3) {
#pragma clang fp contract(off)
        const double sc = ((double)res - 1.0) / (smax[tid][0] - smin[tid][0]);
        hdr->box.scale[tid] = sc;
        hdr->box.translate[tid] = 0.5 - sc * smin[tid][0];
    }
    if (tid == 0) {
        bool ok = n_faces > 0 && !sbad[0];
        for (int c = 0; c < 3; ++c) ok = ok && smax[c][0] > smin[c][0];
        hdr->box.resolution = (double)res;
        hdr->n_refs = 0;
        hdr->n_faces = n_faces;
        hdr->resolution = res;
        hdr->valid = ok ? 1 : 0;
        hdr->status = 0;
        hdr->n_med = 0u;
        hdr->n_huge = 0u;
    }
}

// (int) of a rescaled coordinate, clipped to [0, res - 1]; held to [-1, kCtMaxRes + 1] before it becomes an int (a NaN becomes -1)
__device__ __forceinline__ int ct_clip(double x, int res) {
    const int i = (int)fmin(fmax(x, -1.0), (double)(kCtMaxRes + 1));
    return min(max(i, 0), res - 1);
}

// One lane per face: record, rectangle, class.  Only a VALID mesh gets rectangles: its face ids are in range and its corners finite
__global__ __launch_bounds__(kCtThreads) void k_ct_setup(const float* __restrict__ verts, const int* __restrict__ faces, int n_faces,
                                                         CtHeader* hdr, double* __restrict__ rec, int* __restrict__ rect,
                                                         int* __restrict__ med, int* __restrict__ huge) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * kCtThreads + threadIdx.x;
    if (f >= n_faces) return;
    int* rc = rect + 4 * (size_t)f;
    if (!hdr->valid) {
        rc[0] = 0, rc[1] = -1, rc[2] = 0, rc[3] = -1;
        return;
    }
    const MeshBox bx = hdr->box;
    const int res = hdr->resolution;
    const float* a = verts + 3 * (size_t)faces[3 * (size_t)f];
    const float* b = verts + 3 * (size_t)faces[3 * (size_t)f + 1];
    const float* c = verts + 3 * (size_t)faces[3 * (size_t)f + 2];
    const double t1x = bx.scale[0] * (double)a[0] + bx.translate[0], t1y = bx.scale[1] * (double)a[1] + bx.translate[1],
                 t1z = bx.scale[2] * (double)a[2] + bx.translate[2];
    const double t2x = bx.scale[0] * (double)b[0] + bx.translate[0], t2y = bx.scale[1] * (double)b[1] + bx.translate[1],
                 t2z = bx.scale[2] * (double)b[2] + bx.translate[2];
    const double t3x = bx.scale[0] * (double)c[0] + bx.translate[0], t3y = bx.scale[1] * (double)c[1] + bx.translate[1],
                 t3z = bx.scale[2] * (double)c[2] + bx.translate[2];
    const double A00 = t1x - t3x, A01 = t2x - t3x, A10 = t1y - t3y, A11 = t2y - t3y;
    const double detA = A00 * A11 - A01 * A10;
    const double v1x = t3x - t1x, v1y = t3y - t1y, v1z = t3z - t1z;
    const double v2x = t2x - t1x, v2y = t2y - t1y, v2z = t2z - t1z;
    const double nx = v1y * v2z - v1z * v2y, ny = v1z * v2x - v1x * v2z, nz = v1x * v2y - v1y * v2x;
    const double an = fabs(nz);
    double* r = rec + (size_t)kCtRec * f;
    r[0] = t3x, r[1] = t3y, r[2] = A00, r[3] = A01, r[4] = A10, r[5] = A11;
    r[6] = detA > 0.0 ? 1.0 : -1.0;
    r[7] = fabs(detA);               // 0: no point passes 0 < u < 0
    r[8] = nx, r[9] = ny, r[10] = t1x, r[11] = t1y;
    r[12] = t1z * an;
    r[13] = nz > 0.0 ? 1.0 : -1.0;
    r[14] = an;
    r[15] = 0.0;
    const int ix0 = ct_clip(fmin(t1x, fmin(t2x, t3x)), res), ix1 = ct_clip(fmax(t1x, fmax(t2x, t3x)), res);
    const int iy0 = ct_clip(fmin(t1y, fmin(t2y, t3y)), res), iy1 = ct_clip(fmax(t1y, fmax(t2y, t3y)), res);
    rc[0] = ix0, rc[1] = ix1, rc[2] = iy0, rc[3] = iy1;
    const int n = (ix1 - ix0 + 1) * (iy1 - iy0 + 1);   // <= 4096^2
    if (n > kCtWaveCells) {
        const bool is_huge = n > kCtGroupCells;
        const unsigned slot = atomicAdd(is_huge ? &hdr->n_huge : &hdr->n_med, 1u);   // at most n_faces increments
        if (slot < (unsigned)n_faces) (is_huge ? huge : med)[slot] = f;
    }
}

// the 2-D test of the rule for the record r and the rescaled (qx, qy): true when the column crosses the triangle's interior and
// the triangle is not vertical; then depth and an = |n_z| for the comparison depth >= q.z * an
__device__ __forceinline__ bool ct_test2d(const double* __restrict__ r, double qx, double qy, double& depth, double& an) {
#pragma clang fp contract(off)
    const double t3x = r[0], t3y = r[1], A00 = r[2], A01 = r[3], A10 = r[4], A11 = r[5], s = r[6], ad = r[7];
    const double yx = qx - t3x, yy = qy - t3y;
    const double u = (A11 * yx - A01 * yy) * s, v = (-A10 * yx + A00 * yy) * s;
    const double suv = u + v;
    if (!(0.0 < u && u < ad && 0.0 < v && v < ad && 0.0 < suv && suv < ad)) return false;
    an = r[14];
    if (!(an != 0.0)) return false;
    const double alpha = r[8] * (r[10] - qx) + r[9] * (r[11] - qy);
    depth = r[12] + alpha * r[13];
    return true;
}

// Cells first, first + stride, ... of the rectangle rc (row-major with iy fastest, like the cell index res * ix + iy).
// FILL = false: +1 on the cell's count.  FILL = true: the face claims a slot of the cell; cnt holds the cursors, which started at
// start[cell].  ix <= ix1 < res and iy <= iy1 < res by ct_clip, so the cell lies inside the res^2 cells; a slot is written only
// below n_refs
template <bool FILL>
__device__ __forceinline__ void ct_walk(int ix0, int iy0, int h, int f, unsigned first, unsigned last, unsigned stride, int res,
                                        unsigned* __restrict__ cnt, int* __restrict__ refs, unsigned n_refs) {
    // terminates: last - p strictly decreases (stride >= 1); p + stride <= 2^24 + 2^16 does not wrap
    for (unsigned p = first; p < last; p += stride) {
        const unsigned row = p / (unsigned)h;
        const size_t cell = (size_t)res * (size_t)(ix0 + (int)row) + (size_t)(iy0 + (int)(p - row * (unsigned)h));
        const unsigned slot = atomicAdd(&cnt[cell], 1u);
        if (FILL && slot < n_refs) refs[slot] = f;
    }
}

template <bool FILL>
__global__ __launch_bounds__(kCtThreads) void k_ct_walk(const int* __restrict__ rect, int n_faces, int res, unsigned* __restrict__ cnt,
                                                        int* __restrict__ refs, unsigned n_refs) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const unsigned lane = threadIdx.x & 63;
    // terminates: end - f strictly decreases.  The face count is rounded up to whole waves and step is a multiple of 64, so all 64
    // lanes of a wave reach the ballot together; lanes beyond the end carry no face
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        int ix0 = 0, iy0 = 0, h = 1, n = 0;
        if (f < n_faces) {
            const int* rc = rect + 4 * (size_t)f;
            ix0 = rc[0], iy0 = rc[2], h = rc[3] - rc[2] + 1;
            n = (rc[1] - rc[0] + 1) * h;
            if (rc[1] < rc[0] || h < 1) n = 0, h = 1;
        }
        if (n > 0 && n <= kCtLaneCells) ct_walk<FILL>(ix0, iy0, h, (int)f, 0u, (unsigned)n, 1u, res, cnt, refs, n_refs);
        mesh_wave_turns(n > kCtLaneCells && n <= kCtWaveCells, [&](int src) {
            const int bx0 = __shfl(ix0, src), by0 = __shfl(iy0, src), bh = __shfl(h, src), bn = __shfl(n, src);
            // the lanes of one wave hold 64 consecutive faces: the source lane's is f - lane + src
            ct_walk<FILL>(bx0, by0, bh, (int)(f - lane + src), lane, (unsigned)bn, 64u, res, cnt, refs, n_refs);
        });
    }
}

template <bool FILL>
__global__ __launch_bounds__(kCtThreads) void k_ct_walk_lists(const CtHeader* __restrict__ hdr, const int* __restrict__ rect,
                                                              const int* __restrict__ med, const int* __restrict__ huge, int n_faces,
                                                              int res, unsigned* __restrict__ cnt, int* __restrict__ refs,
                                                              unsigned n_refs) {
    mesh_list_walk<kCtParts, kCtThreads, CtRect>(
        med, min(hdr->n_med, (unsigned)n_faces), huge, min(hdr->n_huge, (unsigned)n_faces),
        [&](int f, CtRect& r) {
            if ((unsigned)f >= (unsigned)n_faces) return 0u;
            const int* rc = rect + 4 * (size_t)f;
            const int h = rc[3] - rc[2] + 1, w = rc[1] - rc[0] + 1;
            if (h < 1 || w < 1) return 0u;
            r.ix0 = rc[0], r.iy0 = rc[2], r.h = h;
            return (unsigned)(w * h);
        },
        [&](int f, const CtRect& r, unsigned first, unsigned last, unsigned stride) {
            ct_walk<FILL>(r.ix0, r.iy0, r.h, f, first, last, stride, res, cnt, refs, n_refs);
        });
}

// ---- exclusive scan of the res^2 counts: block sums, their scan, the starts
__global__ __launch_bounds__(kCtThreads) void k_ct_scan_a(const unsigned* __restrict__ cnt, long long n_cells,
                                                          unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s[kCtThreads];
    const long long base = ((long long)blockIdx.x * kCtThreads + threadIdx.x) * kCtScanPer;
    unsigned long long t = 0;
    for (int u = 0; u < kCtScanPer; ++u)
        if (base + u < n_cells) t += cnt[base + u];
    s[threadIdx.x] = t;
    __syncthreads();
    for (int d = kCtThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] += s[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = s[0];
}

// one workgroup: sums[b] -> the sum of the blocks before b; the total and its verdict to the header
__global__ __launch_bounds__(kCtThreads) void k_ct_scan_b(unsigned long long* __restrict__ sums, int n_blocks, CtHeader* hdr) {
    __shared__ unsigned long long s[kCtThreads];
    const int per = (n_blocks + kCtThreads - 1) / kCtThreads, b0 = threadIdx.x * per, b1 = min(n_blocks, b0 + per);
    unsigned long long t = 0;
    for (int b = b0; b < b1; ++b) t += sums[b];
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < kCtThreads; ++i) {
            const unsigned long long v = s[i];
            s[i] = run;
            run += v;
        }
        hdr->n_refs = (long long)run;   // <= 2^24 cells * 2^28 faces: fits
        if (run > 0x7fffffffull) hdr->status |= 1;
    }
    __syncthreads();
    unsigned long long run = s[threadIdx.x];
    for (int b = b0; b < b1; ++b) {
        const unsigned long long v = sums[b];
        sums[b] = run;
        run += v;
    }
}

// start[c] = references before cell c (modulo 2^32: only used when the total fits), the same into cnt as the fill's cursor
__global__ __launch_bounds__(kCtThreads) void k_ct_scan_c(unsigned* __restrict__ cnt, long long n_cells,
                                                          const unsigned long long* __restrict__ sums, unsigned* __restrict__ start,
                                                          const CtHeader* __restrict__ hdr) {
    __shared__ unsigned long long s[kCtThreads];
    const long long base = ((long long)blockIdx.x * kCtThreads + threadIdx.x) * kCtScanPer;
    unsigned c[kCtScanPer];
    unsigned long long t = 0;
    for (int u = 0; u < kCtScanPer; ++u) {
        c[u] = base + u < n_cells ? cnt[base + u] : 0u;
        t += c[u];
    }
    s[threadIdx.x] = t;
    __syncthreads();
    for (int d = 1; d < kCtThreads; d <<= 1) {   // inclusive scan over the workgroup's threads
        const unsigned long long v = (int)threadIdx.x >= d ? s[threadIdx.x - d] : 0ull;
        __syncthreads();
        s[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = sums[blockIdx.x] + s[threadIdx.x] - t;
    for (int u = 0; u < kCtScanPer; ++u) {
        if (base + u < n_cells) {
            start[base + u] = (unsigned)run;
            cnt[base + u] = (unsigned)run;
        }
        run += c[u];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) start[n_cells] = (unsigned)hdr->n_refs;
}

// the fill restarts the cursors, so that it may run again on the same index
__global__ __launch_bounds__(kCtThreads) void k_ct_cursor(const unsigned* __restrict__ start, long long n_cells, unsigned* __restrict__ cnt) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_cells - c strictly decreases
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < n_cells; c += step) cnt[c] = start[c];
}

// the list [s, e) of the cell ((int)qx, (int)qy) of a rescaled point; empty when the cell is outside [0, res) -- a coordinate equal
// to res, which is in the box, or a NaN (held to -1 before it becomes an int).  Held inside the n_refs references whatever start says
__device__ __forceinline__ void ct_cell_list(const unsigned* __restrict__ start, int res, double qx, double qy, unsigned n_refs,
                                             unsigned& s, unsigned& e) {
    const int cx = (int)fmin(fmax(qx, -1.0), (double)(kCtMaxRes + 1)), cy = (int)fmin(fmax(qy, -1.0), (double)(kCtMaxRes + 1));
    s = e = 0u;
    if (cx < 0 || cx >= res || cy < 0 || cy >= res) return;
    const size_t cell = (size_t)res * cx + cy;
    e = min(start[cell + 1], n_refs);
    s = min(start[cell], e);
}

// ---- one lane per point walks its cell's list
template <typename TP>
__global__ __launch_bounds__(kCtThreads) void k_ct_points(const CtHeader* __restrict__ hdr, const double* __restrict__ rec,
                                                          const unsigned* __restrict__ start, const int* __restrict__ refs,
                                                          unsigned n_refs, int n_faces, const TP* __restrict__ pts, int n_pts,
                                                          uint8_t* __restrict__ inside, uint8_t* __restrict__ ambiguous,
                                                          int* __restrict__ tested) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kCtThreads + threadIdx.x;
    if (i >= n_pts) return;
    const MeshBox bx = hdr->box;
    const int res = hdr->resolution;
    const double R = bx.resolution;
    const double qx = bx.scale[0] * (double)pts[(size_t)i * 3] + bx.translate[0];
    const double qy = bx.scale[1] * (double)pts[(size_t)i * 3 + 1] + bx.translate[1];
    const double qz = bx.scale[2] * (double)pts[(size_t)i * 3 + 2] + bx.translate[2];
    const bool usable = hdr->valid && hdr->n_refs == (long long)n_refs;
    const bool in_box = usable && 0.0 <= qx && qx <= R && 0.0 <= qy && qy <= R && 0.0 <= qz && qz <= R;
    int n0 = 0, n1 = 0;
    unsigned s = 0u, e = 0u;
    if (usable) ct_cell_list(start, res, qx, qy, n_refs, s, e);
    if (in_box) {
        // terminates: e - j strictly decreases
        for (unsigned j = s; j < e; ++j) {
            const int f = refs[j];
            if ((unsigned)f >= (unsigned)n_faces) continue;
            double depth, an;
            if (!ct_test2d(rec + (size_t)kCtRec * f, qx, qy, depth, an)) continue;
            if (depth >= qz * an) ++n0;
            else ++n1;
        }
    }
    inside[i] = (in_box && (n0 & 1) && (n1 & 1)) ? 1 : 0;
    if (ambiguous) ambiguous[i] = (in_box && ((n0 ^ n1) & 1)) ? 1 : 0;
    if (tested) tested[i] = (int)(e - s);   // the candidates of the point's cell, in the box or not
}

// ---- a lattice: one wave (a workgroup of 64 threads) per column (i, j) and per kCtGridZ points of it.  The 2-D test runs once per
// (column, candidate): 64 candidates a round, one per lane; the passing ones' (depth, |n_z|) are packed into LDS, then every lane
// flips the two parities of each of its lattice points k = z0 + 64 m + lane, bit m of n0 / n1.  Nothing is capped: lists of any
// length take more rounds, columns of any height more workgroups (blockIdx.y).  The barriers are met by all 64 threads: every
// trip count depends on the column alone
__global__ __launch_bounds__(64) void k_ct_grid(const CtHeader* __restrict__ hdr, const double* __restrict__ rec,
                                                const unsigned* __restrict__ start, const int* __restrict__ refs, unsigned n_refs,
                                                int n_faces, const float* __restrict__ xs, const float* __restrict__ ys, int ny,
                                                const float* __restrict__ zs, int nz, uint8_t* __restrict__ occ,
                                                unsigned long long* __restrict__ amb) {
#pragma clang fp contract(off)
    __shared__ double s_depth[64], s_an[64];
    const unsigned lane = threadIdx.x;
    const long long col = blockIdx.x;                       // < nx * ny by the launch
    const int i = (int)(col / ny), j = (int)(col - (long long)i * ny);
    const int z0 = blockIdx.y * kCtGridZ;                   // < nz by the launch
    const int rounds_z = (min(nz - z0, kCtGridZ) + 63) / 64;   // 1 .. 64
    const MeshBox bx = hdr->box;
    const int res = hdr->resolution;
    const double R = bx.resolution;
    const double qx = bx.scale[0] * (double)xs[i] + bx.translate[0];
    const double qy = bx.scale[1] * (double)ys[j] + bx.translate[1];
    const bool in_xy = hdr->valid && hdr->n_refs == (long long)n_refs && 0.0 <= qx && qx <= R && 0.0 <= qy && qy <= R;
    unsigned s = 0u, e = 0u;
    if (in_xy) ct_cell_list(start, res, qx, qy, n_refs, s, e);
    unsigned long long n0 = 0ull, n1 = 0ull;
    // terminates: e - base strictly decreases
    for (unsigned base = s; base < e; base += 64u) {
        bool pass = false;
        double depth = 0.0, an = 0.0;
        if (base + lane < e) {
            const int f = refs[base + lane];
            if ((unsigned)f < (unsigned)n_faces) pass = ct_test2d(rec + (size_t)kCtRec * f, qx, qy, depth, an);
        }
        const unsigned long long mask = __ballot(pass);
        const int cnt = __popcll(mask);
        if (pass) {
            const int pos = __popcll(mask & ((1ull << lane) - 1ull));   // < 64
            s_depth[pos] = depth;
            s_an[pos] = an;
        }
        __syncthreads();
        if (cnt)
            for (int m = 0; m < rounds_z; ++m) {
                const int k = z0 + 64 * m + (int)lane;
                if (k >= nz) continue;
                const double qz = bx.scale[2] * (double)zs[k] + bx.translate[2];
                unsigned b0 = 0u, b1 = 0u;
                for (int t = 0; t < cnt; ++t) {
                    if (s_depth[t] >= qz * s_an[t]) b0 ^= 1u;
                    else b1 ^= 1u;
                }
                n0 ^= (unsigned long long)b0 << m;
                n1 ^= (unsigned long long)b1 << m;
            }
        __syncthreads();
    }
    unsigned n_amb = 0u;
    for (int m = 0; m < rounds_z; ++m) {
        const int k = z0 + 64 * m + (int)lane;
        bool is_amb = false;
        if (k < nz) {
            const double qz = bx.scale[2] * (double)zs[k] + bx.translate[2];
            const bool in_box = in_xy && 0.0 <= qz && qz <= R;
            const bool o0 = (n0 >> m) & 1ull, o1 = (n1 >> m) & 1ull;
            occ[(size_t)col * nz + k] = (in_box && o0 && o1) ? 1 : 0;
            is_amb = in_box && o0 != o1;
        }
        n_amb += (unsigned)__popcll(__ballot(is_amb));
    }
    if (amb && lane == 0 && n_amb) atomicAdd(amb, (unsigned long long)n_amb);
}

}  // namespace

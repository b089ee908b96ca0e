// meshwinding.hpp -- generalized winding numbers of a triangle mesh, evaluated hierarchically (Barill et al. 2018, "Fast winding
// numbers for soups and clouds", first order): exact solid angles for the triangles of near leaves, one dipole for a far cluster.
// No reference counterpart; the rule is meshing.winding_tree / meshing.mesh_winding.  float64 throughout, rounded operation by
// operation: contraction is switched off INSIDE every helper the rule's arithmetic runs in (the pragma does not reach a helper that
// is inlined into a function carrying it).  Every integer table equals the rule's, every float table equals it bit for bit, every
// near / far decision and every dipole term too (sqrt and division in float64 are correctly rounded); only atan2 may differ, by its
// last bits.
//
// The index, one launch per line (arah_winding_index_count):
//
//   k_wn_box      lo / side of the cube over the used vertices, validity, the signed volume and its sign -> header (one workgroup)
//   k_wn_keys     one lane per face: the leaf cell of its centroid, the cell's Morton key, +1 on the cell's count (integer atomicAdd)
//   k_wn_scan     exclusive scan of the 8^depth counts -> the cells' starts (one workgroup: at most 2^21 cells)
//   k_wn_fill     every face claims a slot of its cell, in the order of arrival
//   k_wn_rank     ... and is then ranked among its cell's faces by id: the list is ordered by (key, face id) whatever the arrival
//   k_wn_heads    the level at which a triangle of the list starts a node, and how many nodes start there
//   k_wn_scan     exclusive scan of those numbers -> the preorder number of every node; the total (64-bit) goes to the header
//
// The caller reads the number of nodes from the header -- the index's ONE host synchronisation --, allocates the node tables, and
// arah_winding_index_fill writes them: k_wn_nodes (first, count, level, skip), k_wn_leaf (a leaf's sums, its members in list order,
// by one lane), k_wn_inner level by level upwards (a node's sums, its children in child order), k_wn_centroid, k_wn_radius (one wave
// per node: a maximum does not depend on the order).  Integer atomics only.  No thread waits for another; every loop ends by an
// argument stated at the loop.  Included by arah_hip.hip after meshsdf.hpp.
#pragma once

namespace {

constexpr int kWnThreads = 256;
constexpr int kWnScanThreads = 1024;
constexpr int kWnMaxDepth = 7;            // 21 bits of key
constexpr int kWnMaxFaces = 1 << 28;
constexpr unsigned kWnMaxLeaf = 1u << 15;  // faces of one leaf cell at depth > 0: k_wn_rank is quadratic in a cell (meshing.WINDING_MAX_LEAF)
constexpr int kWnNodeF = 8;               // doubles of a node: centroid xyz, radius, area vector xyz, area
constexpr int kWnNodeI = 4;               // ints of a node: first, count, level, skip
constexpr double kWnFourPi = 12.566370614359172;   // 4.0 * M_PI, rounded once

struct WnHeader {
    double lo[3];                // offset 0
    double side;                 // 24
    double volume;               // 32
    long long n_nodes;           // 40
    int n_faces, depth;          // 48, 52
    int valid;                   // 56: every used vertex is finite
    int status;                  // 60: bit 0 = a face id outside [0, V); bit 1 = a leaf cell with more than kWnMaxLeaf faces
    int orient;                  // 64: +1 / -1
    int pad;
};

struct WnIndex {
    WnHeader* hdr;
    unsigned* key;               // [F] the leaf key of face f
    unsigned* skey;              // [F] the keys in list order
    int* tmp;                    // [F] the faces by cell, in the order of arrival
    int* hlev;                   // [F] the level at which list entry i starts a node (depth + 1: none)
    long long* cnt64;            // [F] nodes that start at list entry i
    long long* prefix;           // [F + 1] their exclusive scan
    unsigned* ccnt;              // [8^depth] counts, then the fill's cursors
    unsigned* cstart;            // [8^depth + 1]
    size_t bytes;
};

// THE rule of depth = auto, meshing.winding_depth: the smallest depth with 8 * 4^depth >= n_faces (about eight triangles a leaf of a
// surface), chosen from the depth sweep of tools/mesh_winding_bench.py
inline int wn_auto_depth(int n_faces) {
    int d = 0;
    while (d < kWnMaxDepth && (8ll << (2 * d)) < (long long)n_faces) ++d;
    return d;
}

// corner k of face f as doubles; a face id outside [0, V) reads vertex 0 or V - 1 (the mesh is then refused by its status)
__device__ __forceinline__ void wn_corner(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, long long f, int k,
                                          double* out) {
    const int v = min(max(faces[3 * f + k], 0), n_verts - 1);
    for (int c = 0; c < 3; ++c) out[c] = (double)verts[(size_t)v * 3 + c];
}

// bit b of ix, iy, iz -> bits 3b + 2, 3b + 1, 3b
__device__ __forceinline__ unsigned wn_morton(unsigned ix, unsigned iy, unsigned iz, int depth) {
    unsigned key = 0u;
    for (int b = 0; b < depth; ++b)
        key |= (((ix >> b) & 1u) << (3 * b + 2)) | (((iy >> b) & 1u) << (3 * b + 1)) | (((iz >> b) & 1u) << (3 * b));
    return key;
}

__device__ __forceinline__ double wn_dot3(const double* u, const double* v) {
#pragma clang fp contract(off)
    return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}

// u . (v x w), the cross product first, the dot product summed from the left
__device__ __forceinline__ double wn_det3(const double* u, const double* v, const double* w) {
#pragma clang fp contract(off)
    const double crx = v[1] * w[2] - v[2] * w[1];
    const double cry = v[2] * w[0] - v[0] * w[2];
    const double crz = v[0] * w[1] - v[1] * w[0];
    return (u[0] * crx + u[1] * cry) + u[2] * crz;
}

// the centroid ((a + b) + c) / 3
__device__ __forceinline__ void wn_centroid3(const double* a, const double* b, const double* c, double* g) {
#pragma clang fp contract(off)
    for (int k = 0; k < 3; ++k) g[k] = ((a[k] + b[k]) + c[k]) / 3.0;
}

// lo / side, validity, orientation.  The signed volume: partial sum t takes the faces t, t + 256, ... in ascending order, then
// p[t] += p[t + s] for s = 128 .. 1 -- the order meshing.winding_orient states; it rides along in the rounds of mesh_box_reduce
__global__ __launch_bounds__(kWnThreads) void k_wn_box(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                       int n_faces, int depth, WnHeader* hdr) {
#pragma clang fp contract(off)
    static_assert(kWnThreads == kBoxThreads, "mesh_box_reduce");
    __shared__ double smin[3][kWnThreads], smax[3][kWnThreads], svol[kWnThreads];
    __shared__ int sbad[kWnThreads];
    const int tid = threadIdx.x;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, vol = 0.0;
    int bad = 0;
    // terminates: n_faces - f strictly decreases
    for (long long f = tid; f < n_faces; f += kWnThreads) {
        double p[3][3];
        for (int k = 0; k < 3; ++k) {
            if ((unsigned)faces[3 * f + k] >= (unsigned)n_verts) bad |= 1;
            wn_corner(verts, n_verts, faces, f, k, p[k]);
            for (int c = 0; c < 3; ++c) {
                if (!isfinite(p[k][c])) bad |= 2;
                lo[c] = fmin(lo[c], p[k][c]);
                hi[c] = fmax(hi[c], p[k][c]);
            }
        }
        vol = vol + wn_det3(p[0], p[1], p[2]);
    }
    svol[tid] = vol;   // visible to the first round through the barrier in front of it
    mesh_box_reduce(lo, hi, bad, smin, smax, sbad, [&](int s) { svol[tid] = svol[tid] + svol[tid + s]; });
    if (tid == 0) {
        const double ex = smax[0][0] - smin[0][0], ey = smax[1][0] - smin[1][0], ez = smax[2][0] - smin[2][0];
        const double volume = svol[0] / 6.0;
        for (int c = 0; c < 3; ++c) hdr->lo[c] = n_faces > 0 ? smin[c][0] : 0.0;
        hdr->side = n_faces > 0 ? fmax(ex, fmax(ey, ez)) : 0.0;
        hdr->volume = volume;
        hdr->n_nodes = 0;
        hdr->n_faces = n_faces;
        hdr->depth = depth;
        hdr->valid = (sbad[0] & 2) ? 0 : 1;
        hdr->status = sbad[0] & 1;
        hdr->orient = volume < 0.0 ? -1 : 1;
        hdr->pad = 0;
    }
}

// the leaf cell of a face's centroid: i = (int) clamp((g - lo) * (2^depth / side), 0, 2^depth - 1), a NaN counting as 0
__global__ __launch_bounds__(kWnThreads) void k_wn_keys(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, int depth, const WnHeader* __restrict__ hdr,
                                                        unsigned* __restrict__ key, unsigned* __restrict__ ccnt) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * kWnThreads + threadIdx.x;
    if (f >= n_faces) return;
    double a[3], b[3], c[3], g[3];
    wn_corner(verts, n_verts, faces, f, 0, a);
    wn_corner(verts, n_verts, faces, f, 1, b);
    wn_corner(verts, n_verts, faces, f, 2, c);
    wn_centroid3(a, b, c, g);
    const double top = (double)((1 << depth) - 1);
    const double inv = (double)(1 << depth) / hdr->side;
    unsigned cell[3];
    for (int k = 0; k < 3; ++k) {
        const double q = (g[k] - hdr->lo[k]) * inv;
        cell[k] = (unsigned)(int)fmin(fmax(q, 0.0), top);   // fmax(NaN, 0) = 0; the value lies in [0, 2^depth - 1]
    }
    const unsigned k = wn_morton(cell[0], cell[1], cell[2], depth);   // < 8^depth
    key[f] = k;
    atomicAdd(&ccnt[k], 1u);
}

// exclusive scan by one workgroup: out[i] = in[0] + .. + in[i - 1], out[n] = the total; cursor (or NULL) receives out[0 .. n) too
// and may be the input itself (every element is read before it is written, by the same thread)
template <typename TI, typename TO>
__global__ __launch_bounds__(kWnScanThreads) void k_wn_scan(const TI* in, long long n, TO* out, TI* cursor, long long* total) {
    __shared__ unsigned long long s[kWnScanThreads];
    const long long per = (n + kWnScanThreads - 1) / kWnScanThreads;
    const long long b0 = min(n, (long long)threadIdx.x * per), b1 = min(n, b0 + per);
    unsigned long long t = 0;
    for (long long b = b0; b < b1; ++b) t += (unsigned long long)in[b];   // terminates: b1 - b strictly decreases
    s[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < kWnScanThreads; ++i) {
            const unsigned long long v = s[i];
            s[i] = run;
            run += v;
        }
        out[n] = (TO)run;
        if (total) *total = (long long)run;   // <= 2^28 faces * 8 levels: fits
    }
    __syncthreads();
    unsigned long long run = s[threadIdx.x];
    for (long long b = b0; b < b1; ++b) {
        const unsigned long long v = (unsigned long long)in[b];
        out[b] = (TO)run;
        if (cursor) cursor[b] = (TI)run;
        run += v;
    }
}

__global__ __launch_bounds__(kWnThreads) void k_wn_fill(const unsigned* __restrict__ key, int n_faces, unsigned n_cells,
                                                        unsigned* __restrict__ cursor, int* __restrict__ tmp) {
    const int f = blockIdx.x * kWnThreads + threadIdx.x;
    if (f >= n_faces) return;
    const unsigned k = key[f];
    if (k >= n_cells) return;
    const unsigned slot = atomicAdd(&cursor[k], 1u);   // the cursors started at cstart: slot < cstart[k + 1] <= n_faces
    if (slot < (unsigned)n_faces) tmp[slot] = f;
}

// slot s of the arrival order holds face f of cell k: its place in the list is cstart[k] + the number of the cell's faces with a
// smaller id.  With depth 0 the one cell holds every face and that number is f itself.  Writes the list, its keys and its corners.
// The ranking is quadratic in a cell, so a cell with more than kWnMaxLeaf faces is REFUSED: its faces keep the order of arrival
// (slot s lies in the cell's own range), status bit 1 is raised and the mesh is marked not valid -- every winding number is NaN
__global__ __launch_bounds__(kWnThreads) void k_wn_rank(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                        int n_faces, int depth, const unsigned* __restrict__ key,
                                                        const unsigned* __restrict__ cstart, const int* __restrict__ tmp,
                                                        int* __restrict__ order, unsigned* __restrict__ skey, float* __restrict__ tris,
                                                        WnHeader* hdr) {
    const int s = blockIdx.x * kWnThreads + threadIdx.x;
    if (s >= n_faces) return;
    const int f = tmp[s];
    if ((unsigned)f >= (unsigned)n_faces) return;
    const unsigned k = key[f];
    const unsigned c0 = min(cstart[k], (unsigned)n_faces), c1 = min(cstart[k + 1], (unsigned)n_faces);
    unsigned rank = 0u;
    if (depth == 0) {
        rank = (unsigned)f;
    } else if (c1 - c0 > kWnMaxLeaf) {
        rank = (unsigned)s - c0;      // refused: the order of arrival
        if (rank == 0u) {
            atomicOr(&hdr->status, 2);
            atomicAnd(&hdr->valid, 0);
        }
    } else {
        for (unsigned j = c0; j < c1; ++j) rank += tmp[j] < f ? 1u : 0u;   // terminates: c1 - j strictly decreases (<= kWnMaxLeaf trips)
    }
    const unsigned pos = c0 + rank;   // < c1 <= n_faces: at most c1 - c0 - 1 ids of the cell are smaller
    if (pos >= (unsigned)n_faces) return;
    order[pos] = f;
    skey[pos] = k;
    for (int c = 0; c < 3; ++c) {
        const int v = min(max(faces[3 * (size_t)f + c], 0), n_verts - 1);
        for (int d = 0; d < 3; ++d) tris[(size_t)pos * 9 + 3 * c + d] = verts[(size_t)v * 3 + d];
    }
}

// list entry i starts a node at every level >= h: h = 0 for the first, depth - (highest differing bit) / 3 against its predecessor,
// depth + 1 (no node) where the key repeats
__global__ __launch_bounds__(kWnThreads) void k_wn_heads(const unsigned* __restrict__ skey, int n_faces, int depth, int* __restrict__ hlev,
                                                         long long* __restrict__ cnt64) {
    const int i = blockIdx.x * kWnThreads + threadIdx.x;
    if (i >= n_faces) return;
    int h = 0;
    if (i > 0) {
        const unsigned x = skey[i] ^ skey[i - 1];
        h = x ? depth - (31 - __clz((int)x)) / 3 : depth + 1;
        h = min(max(h, 0), depth + 1);
    }
    hlev[i] = h;
    cnt64[i] = depth + 1 - h;
}

// the first list entry whose key is >= target
__device__ __forceinline__ int wn_lower_bound(const unsigned* __restrict__ skey, int n, unsigned long long target) {
    int lo = 0, hi = n;
    while (lo < hi) {   // terminates: hi - lo strictly decreases
        const int mid = lo + (hi - lo) / 2;
        if ((unsigned long long)skey[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kWnThreads) void k_wn_nodes(const unsigned* __restrict__ skey, const int* __restrict__ hlev,
                                                         const long long* __restrict__ prefix, int n_faces, int depth, int n_nodes,
                                                         int* __restrict__ node_i) {
    const int i = blockIdx.x * kWnThreads + threadIdx.x;
    if (i >= n_faces) return;
    const int h = hlev[i];
    const unsigned k = skey[i];
    for (int l = max(h, 0); l <= depth; ++l) {
        const long long node = prefix[i] + (l - h);
        if (node < 0 || node >= n_nodes) continue;
        const int s = 3 * (depth - l);
        const int end = wn_lower_bound(skey, n_faces, (((unsigned long long)k >> s) + 1ull) << s);   // > i: entry i is below the target
        int* ni = node_i + (size_t)kWnNodeI * node;
        ni[0] = i;
        ni[1] = end - i;
        ni[2] = l;
        ni[3] = (int)min(prefix[end], (long long)n_nodes);   // prefix[F] = the number of nodes
    }
}

// area vector ((b - a) x (c - a)) / 2, its length, the centroid: what a triangle adds to its leaf
__device__ __forceinline__ void wn_moments(const float* __restrict__ t, double* nv, double& area, double* g) {
#pragma clang fp contract(off)
    double a[3], b[3], c[3], e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)t[k], b[k] = (double)t[3 + k], c[k] = (double)t[6 + k];
        e1[k] = b[k] - a[k];
        e2[k] = c[k] - a[k];
    }
    nv[0] = 0.5 * (e1[1] * e2[2] - e1[2] * e2[1]);
    nv[1] = 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]);
    nv[2] = 0.5 * (e1[0] * e2[1] - e1[1] * e2[0]);
    area = sqrt(wn_dot3(nv, nv));
    wn_centroid3(a, b, c, g);
}

// one lane per leaf: n, area and area * g over its members in list order, from 0.  Until k_wn_centroid runs, slots 0..2 of a node
// hold the sum of area * g
__global__ __launch_bounds__(kWnThreads) void k_wn_leaf(const int* __restrict__ hlev, const long long* __restrict__ prefix,
                                                        const float* __restrict__ tris, int n_faces, int depth, int n_nodes,
                                                        const int* __restrict__ node_i, double* __restrict__ node_f) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kWnThreads + threadIdx.x;
    if (i >= n_faces) return;
    const int h = hlev[i];
    if (h > depth) return;
    const long long node = prefix[i] + (depth - h);
    if (node < 0 || node >= n_nodes) return;
    const int end = min(n_faces, i + max(node_i[(size_t)kWnNodeI * node + 1], 0));
    double sn[3] = {0.0, 0.0, 0.0}, sa = 0.0, sg[3] = {0.0, 0.0, 0.0};
    for (int t = i; t < end; ++t) {   // terminates: end - t strictly decreases
        double nv[3], area, g[3];
        wn_moments(tris + (size_t)t * 9, nv, area, g);
        for (int k = 0; k < 3; ++k) {
            sn[k] = sn[k] + nv[k];
            sg[k] = sg[k] + area * g[k];
        }
        sa = sa + area;
    }
    double* nf = node_f + (size_t)kWnNodeF * node;
    nf[0] = sg[0], nf[1] = sg[1], nf[2] = sg[2], nf[3] = 0.0;
    nf[4] = sn[0], nf[5] = sn[1], nf[6] = sn[2], nf[7] = sa;
}

// one lane per node of `level` (< depth): its children's sums in child order, from 0.  The children are the nodes of level + 1
// from node + 1 on, each reached by its predecessor's skip
__global__ __launch_bounds__(kWnThreads) void k_wn_inner(int level, int n_nodes, const int* __restrict__ node_i, double* __restrict__ node_f) {
#pragma clang fp contract(off)
    const int node = blockIdx.x * kWnThreads + threadIdx.x;
    if (node >= n_nodes || node_i[(size_t)kWnNodeI * node + 2] != level) return;
    const int stop = min(node_i[(size_t)kWnNodeI * node + 3], n_nodes);
    double s[kWnNodeF] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int child = node + 1;
    while (child < stop) {   // terminates: child strictly increases (the skip is held above the node)
        const double* cf = node_f + (size_t)kWnNodeF * child;
        for (int k = 0; k < kWnNodeF; ++k) s[k] = s[k] + cf[k];
        child = max(node_i[(size_t)kWnNodeI * child + 3], child + 1);
    }
    double* nf = node_f + (size_t)kWnNodeF * node;
    for (int k = 0; k < kWnNodeF; ++k) nf[k] = s[k];
    nf[3] = 0.0;
}

// centroid = sum(area g) / sum(area) where the area is > 0, else the centre of the node's cell: lo + (i + 0.5) * (side / 2^level)
__global__ __launch_bounds__(kWnThreads) void k_wn_centroid(const WnHeader* __restrict__ hdr, const unsigned* __restrict__ skey, int n_faces,
                                                            int depth, int n_nodes, const int* __restrict__ node_i,
                                                            double* __restrict__ node_f) {
#pragma clang fp contract(off)
    const int node = blockIdx.x * kWnThreads + threadIdx.x;
    if (node >= n_nodes) return;
    const int* ni = node_i + (size_t)kWnNodeI * node;
    double* nf = node_f + (size_t)kWnNodeF * node;
    const double area = nf[7];
    if (area > 0.0) {
        for (int k = 0; k < 3; ++k) nf[k] = nf[k] / area;
        return;
    }
    const int level = min(max(ni[2], 0), depth), first = min(max(ni[0], 0), n_faces - 1);
    const unsigned k = skey[first] >> (3 * (depth - level));
    unsigned cell[3] = {0u, 0u, 0u};
    for (int b = 0; b < level; ++b)
        for (int a = 0; a < 3; ++a) cell[a] |= ((k >> (3 * b + 2 - a)) & 1u) << b;
    const double width = hdr->side / (double)(1 << level);
    for (int a = 0; a < 3; ++a) nf[a] = hdr->lo[a] + ((double)cell[a] + 0.5) * width;
}

__device__ __forceinline__ double wn_dist2(const double* c, double x, double y, double z) {
#pragma clang fp contract(off)
    const double dx = x - c[0], dy = y - c[1], dz = z - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// one wave per node: radius = sqrt(max |corner - centroid|^2) over the corners of its members
__global__ __launch_bounds__(kWnThreads) void k_wn_radius(const float* __restrict__ tris, int n_faces, int n_nodes,
                                                          const int* __restrict__ node_i, double* __restrict__ node_f) {
    const int node = blockIdx.x * (kWnThreads / 64) + (threadIdx.x >> 6);   // the same for all 64 lanes of a wave
    const unsigned lane = threadIdx.x & 63;
    if (node >= n_nodes) return;
    const int* ni = node_i + (size_t)kWnNodeI * node;
    double* nf = node_f + (size_t)kWnNodeF * node;
    const int first = max(ni[0], 0), end = min(n_faces, first + max(ni[1], 0));
    const double c[3] = {nf[0], nf[1], nf[2]};
    double m = 0.0;
    for (int t = first + (int)lane; t < end; t += 64) {   // terminates: end - t strictly decreases
        const float* p = tris + (size_t)t * 9;
        for (int k = 0; k < 3; ++k) m = fmax(m, wn_dist2(c, (double)p[3 * k], (double)p[3 * k + 1], (double)p[3 * k + 2]));
    }
    for (int s = 32; s > 0; s >>= 1) m = fmax(m, __shfl_xor(m, s));
    if (lane == 0) nf[3] = sqrt(m);
}

// ---- the query
// Van Oosterom & Strackee: the solid angle of the triangle t (nine floats) seen from p; meshing.solid_angle_terms
__device__ __forceinline__ double wn_term(const float* __restrict__ t, double px, double py, double pz) {
#pragma clang fp contract(off)
    double a[3], b[3], c[3];
    a[0] = (double)t[0] - px, a[1] = (double)t[1] - py, a[2] = (double)t[2] - pz;
    b[0] = (double)t[3] - px, b[1] = (double)t[4] - py, b[2] = (double)t[5] - pz;
    c[0] = (double)t[6] - px, c[1] = (double)t[7] - py, c[2] = (double)t[8] - pz;
    const double num = wn_det3(a, b, c);
    const double la = sqrt(wn_dot3(a, a)), lb = sqrt(wn_dot3(b, b)), lc = sqrt(wn_dot3(c, c));
    const double den = (((la * lb) * lc + wn_dot3(a, b) * lc) + wn_dot3(b, c) * la) + wn_dot3(c, a) * lb;
    if (num == 0.0) return 0.0;
    return 2.0 * atan2(num, den);
}

// the dipole of a far node: (d . n) / (d2 * sqrt(d2)), d = centroid - p
__device__ __forceinline__ double wn_dipole(const double* __restrict__ nf, double px, double py, double pz, double d2) {
#pragma clang fp contract(off)
    const double d[3] = {nf[0] - px, nf[1] - py, nf[2] - pz};
    return wn_dot3(d, nf + 4) / (d2 * sqrt(d2));
}

// is the node far: |centroid - p|^2 > accuracy^2 * (r * r); d2 goes back to the caller
__device__ __forceinline__ bool wn_is_far(const double* __restrict__ nf, double px, double py, double pz, double acc2, double& d2) {
#pragma clang fp contract(off)
    const double d[3] = {nf[0] - px, nf[1] - py, nf[2] - pz};
    d2 = wn_dot3(d, d);
    const double r = nf[3];
    return d2 > acc2 * (r * r);
}

// the walk of meshing.mesh_winding for one point.  Terminates: the node number strictly increases (a skip is held above its node)
__device__ __forceinline__ double wn_walk(const WnHeader* __restrict__ hdr, const float* __restrict__ tris, int n_faces, int depth,
                                          const int* __restrict__ node_i, const double* __restrict__ node_f, int n_nodes, double acc2,
                                          double px, double py, double pz, int& n_exact, int& n_far) {
#pragma clang fp contract(off)
    n_exact = 0, n_far = 0;
    if (!hdr->valid) return __longlong_as_double(0x7ff8000000000000ll);
    double sum = 0.0;
    int node = 0;
    while (node < n_nodes) {
        const int* ni = node_i + (size_t)kWnNodeI * node;
        const double* nf = node_f + (size_t)kWnNodeF * node;
        const int next = max(ni[3], node + 1);
        double d2;
        if (wn_is_far(nf, px, py, pz, acc2, d2)) {
            sum = sum + wn_dipole(nf, px, py, pz, d2);
            ++n_far;
            node = next;
        } else if (ni[2] >= depth) {
            const int first = max(ni[0], 0), end = min(n_faces, first + max(ni[1], 0));
            for (int t = first; t < end; ++t) sum = sum + wn_term(tris + (size_t)t * 9, px, py, pz);   // terminates: end - t decreases
            n_exact += max(end - first, 0);
            node = next;
        } else {
            ++node;
        }
    }
    return sum / kWnFourPi;
}

__device__ __forceinline__ void wn_store(const WnHeader* __restrict__ hdr, long long i, double wv, int ne, int nf, double* __restrict__ w,
                                         uint8_t* __restrict__ inside, int* __restrict__ n_exact, int* __restrict__ n_far) {
#pragma clang fp contract(off)
    w[i] = wv;
    if (inside) inside[i] = ((double)hdr->orient * wv >= 0.5) ? 1 : 0;   // a NaN is outside
    if (n_exact) n_exact[i] = ne;
    if (n_far) n_far[i] = nf;
}

// one lane per point: each point's sum in the order of the rule, no atomics
__global__ __launch_bounds__(kWnThreads) void k_wn_points(const WnHeader* __restrict__ hdr, const float* __restrict__ tris, int n_faces,
                                                          int depth, const int* __restrict__ node_i, const double* __restrict__ node_f,
                                                          int n_nodes, double acc2, const float* __restrict__ pts, int n_pts,
                                                          double* __restrict__ w, uint8_t* __restrict__ inside,
                                                          int* __restrict__ n_exact, int* __restrict__ n_far) {
    const long long i = (long long)blockIdx.x * kWnThreads + threadIdx.x;
    if (i >= n_pts) return;
    int ne, nf;
    const double wv = wn_walk(hdr, tris, n_faces, depth, node_i, node_f, n_nodes, acc2, (double)pts[i * 3], (double)pts[i * 3 + 1],
                              (double)pts[i * 3 + 2], ne, nf);
    wn_store(hdr, i, wv, ne, nf, w, inside, n_exact, n_far);
}

// one lane per lattice point (ix, iy, iz), iz fastest: the 64 points of a wave are neighbours along z and walk nearly the same nodes
__global__ __launch_bounds__(kWnThreads) void k_wn_grid(const WnHeader* __restrict__ hdr, const float* __restrict__ tris, int n_faces,
                                                        int depth, const int* __restrict__ node_i, const double* __restrict__ node_f,
                                                        int n_nodes, double acc2, const float* __restrict__ xs, const float* __restrict__ ys,
                                                        int ny, const float* __restrict__ zs, int nz, long long n_pts,
                                                        double* __restrict__ w, uint8_t* __restrict__ inside, int* __restrict__ n_exact,
                                                        int* __restrict__ n_far) {
    const long long i = (long long)blockIdx.x * kWnThreads + threadIdx.x;
    if (i >= n_pts) return;
    const long long col = i / nz;
    const int iz = (int)(i - col * nz), ix = (int)(col / ny), iy = (int)(col - (long long)ix * ny);   // ix < nx: i < nx ny nz
    int ne, nf;
    const double wv = wn_walk(hdr, tris, n_faces, depth, node_i, node_f, n_nodes, acc2, (double)xs[ix], (double)ys[iy], (double)zs[iz],
                              ne, nf);
    wn_store(hdr, i, wv, ne, nf, w, inside, n_exact, n_far);
}

}  // namespace

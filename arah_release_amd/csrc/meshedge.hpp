// meshedge.hpp -- the edge toolkit: what the kernels that work on the EDGES of an indexed mesh do with MeshAdj (meshadj.hpp).  The
// round kernels (meshcollapse.hpp, meshsubdiv.hpp, meshflip.hpp) take all of it; meshlaplace.hpp and meshorient.hpp the clamped
// segment and ma_dot.  DESIGN.md ("Indexed meshes: the adjacency view and the edge toolkit") tells the same once.
//
//   ma_fill_owner    owner[i] = the vertex whose segment the neighbour entry i lies in
//   ma_entry         u = owner[i], v = nbr[i] of entry i, and whether it names an edge: every undirected edge once, from its lower end
//   ma_walk, ma_entry_walk   the element-wise walk over the entries in whole waves, without and with the entry's ends
//   ma_segment       a vertex's rows of a CSR that is the caller's, clamped to the array
//   ma_lower         the bisection of ascending ids to a lower bound; ma_find, the entry of b in a's segment
//   MaMerge          the merge of two ascending segments (neighbours of u and v, faces of u and v)
//   ma_finite, ma_load, ma_d2, ma_dot, ma_cross   float64 from float32 vertices, every operation rounded on its own
//
// NOT MEASURED AGAINST AN ALTERNATIVE: the owner array (4 bytes per entry, filled by one thread per vertex) instead of a binary
// search of nbr_start by every lane that needs the owner of its entry.
#pragma once

// The owner of every entry of v's segment.  One thread per vertex calls it from the first kernel of a round (k_mx_pin, k_mf_init,
// k_sb_owner): the view's arrays are the round's own, so the segment needs no clamp.  i < nbr_start[V] <= 6 F
__device__ __forceinline__ void ma_fill_owner(const MeshAdj& adj, long long v, int* __restrict__ owner) {
    const int last = adj.nbr_start[v + 1];
    for (int i = adj.nbr_start[v]; i < last; ++i) owner[i] = (int)v;   // terminates: last - i strictly decreases
}

// entry i < n_entries = nbr_start[V]: its two ends; true when it names an edge (the entry of the higher end does not)
__device__ __forceinline__ bool ma_entry(const MeshAdj& adj, const int* __restrict__ owner, long long i, int& u, int& v) {
    u = owner[i];
    v = adj.nbr[i];
    return v > u;
}

// The walk of one lane per entry: body(i, live), live = i is an entry (i < nbr_start[V]).  THE ENTRY COUNT IS ROUNDED UP TO WHOLE
// WAVES AND EVERY LANE REACHES THE BODY, from wave-uniform control flow, so that the ballots of cc_add_one in it meet; lanes beyond
// the entries, and beyond n_entries_cap (the rows the per-entry outputs have, 6 F), carry live = false and must write nothing
// unless i < n_entries_cap.  k_mx_select and k_sb_marks number their entries instead (mesh_compact, sb_walk: chunks, not strides).
template <class Body>
__device__ __forceinline__ void ma_walk(const MeshAdj& adj, int n_entries_cap, Body body) {
    const int n_entries = adj.nbr_start[adj.n_verts];
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_entries_cap + 63) & ~63ll;
    // terminates: end - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += step) body(i, i < n_entries);
}

// the same walk for the kernels that look at every edge: body(i, is_edge, u, v), u and v valid when is_edge
template <class Body>
__device__ __forceinline__ void ma_entry_walk(const MeshAdj& adj, const int* __restrict__ owner, int n_entries_cap, Body body) {
    ma_walk(adj, n_entries_cap, [&](long long i, bool live) {
        int u = -1, v = -1;
        const bool is_edge = live && ma_entry(adj, owner, i, u, v);
        body(i, is_edge, u, v);
    });
}

// v's rows of a CSR whose starts are the CALLER's, clamped to the rows the array has: 0 <= lo <= hi <= rows
__device__ __forceinline__ void ma_segment(const int* __restrict__ start, long long v, long long rows, long long& lo, long long& hi) {
    lo = min(max((long long)start[v], 0ll), rows);
    hi = min(max((long long)start[v + 1], lo), rows);
}

// the first row of the ascending ids[lo .. hi) that holds a value >= key, hi without one.  Reads rows of [lo, hi) only
template <class Index>
__device__ __forceinline__ Index ma_lower(const int* __restrict__ ids, Index lo, Index hi, int key) {
    while (lo < hi) {   // terminates: hi - lo strictly decreases (lo < mid + 1 <= hi or hi = mid < hi)
        const Index mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the entry (a, b) of an adjacency the round built itself: b in a's ascending neighbour segment, -1 when {a, b} is no edge.
// meshlaplace.hpp (ml_find) and meshorient.hpp (mo_edge_faces) search rows of the CALLER's arrays, which they clamp first
// (ma_segment), and leave their loop at the first equal row: a lower bound there costs the probes down to one row
__device__ __forceinline__ int ma_find(const MeshAdj& adj, int a, int b) {
    const int last = adj.nbr_start[a + 1], at = ma_lower(adj.nbr, adj.nbr_start[a], last, b);
    return at < last && adj.nbr[at] == b ? at : -1;
}

// The merge of two ascending lists without repeats: the values of both, ascending, each once.
struct MaMerge {
    const int *a, *b;
    int i, ni, j, nj;
};

__device__ __forceinline__ MaMerge ma_merge(const int* __restrict__ list, const int* __restrict__ start, int u, int v) {
    return MaMerge{list + start[u], list + start[v], 0, start[u + 1] - start[u], 0, start[v + 1] - start[v]};
}

__device__ __forceinline__ bool ma_more(const MaMerge& w) { return w.i < w.ni || w.j < w.nj; }

// the next value (call it while ma_more); both = it stands in both lists.  Every call consumes at least one element.  The ids
// of faces and vertices lie below INT32_MAX, which stands for an exhausted list
__device__ __forceinline__ int ma_next(MaMerge& w, bool& both) {
    const int x = w.i < w.ni ? w.a[w.i] : INT32_MAX, y = w.j < w.nj ? w.b[w.j] : INT32_MAX;
    both = x == y;
    if (x <= y) ++w.i;
    if (y <= x) ++w.j;
    return min(x, y);
}

// ---- float64 from float32 vertices.  `#pragma clang fp contract(off)` stands in every helper and in every caller that does
// arithmetic of its own: it does not reach across an inlined call.  meshquadric.hpp's mq_term and meshlaplace.hpp's ml_face form
// their differences inline and stay as they are.
__device__ __forceinline__ bool ma_finite(const float* __restrict__ verts, long long v) {
    return isfinite(verts[3 * v + 0]) && isfinite(verts[3 * v + 1]) && isfinite(verts[3 * v + 2]);
}

// vertex x widened; finite is cleared when a coordinate is not finite (and never set)
__device__ __forceinline__ void ma_load(const float* __restrict__ verts, int x, double p[3], bool& finite) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t = verts[3 * (size_t)x + c];
        finite = finite && isfinite(t);
        p[c] = (double)t;
    }
}

// the squared distance of two float32 points in double: (dx dx + dy dy) + dz dz
__device__ __forceinline__ double ma_d2(const float* p, const float* q) {
#pragma clang fp contract(off)
    const double dx = (double)p[0] - (double)q[0], dy = (double)p[1] - (double)q[1], dz = (double)p[2] - (double)q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// (x0 y0 + x1 y1) + x2 y2
__device__ __forceinline__ double ma_dot(const double* x, const double* y) {
#pragma clang fp contract(off)
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// (p1 - p0) x (p2 - p0), the components as mq_term forms them
__device__ __forceinline__ void ma_cross(const double p0[3], const double p1[3], const double p2[3], double n[3]) {
#pragma clang fp contract(off)
    double e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e1[a] = p1[a] - p0[a];
        e2[a] = p2[a] - p0[a];
    }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

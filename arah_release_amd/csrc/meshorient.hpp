// meshorient.hpp -- repair of an indexed mesh on the device: consistent orientation of its faces, its boundary loops, and the
// filling of small holes by a fan around the loop's mean.
//
// Reference: none in its tree.  The reference's users repair scans with trimesh (repair.fix_normals, repair.fill_holes); it is
// no dependency of this project.  Both repairs are integer problems over the adjacency of meshadj.hpp, and every result is
// defined so that it is unique and compared bit for bit with the tensor specification (meshing.mesh_orient /
// mesh_boundary_loops / mesh_fill_holes), where the rules are stated once.  In short:
//
//   * validity and traversal are those of meshadj.hpp; two valid faces are NEIGHBOURS across an undirected edge when exactly two
//     valid faces lie on it, consistent (s = 0) when they traverse it in opposite directions, inconsistent (s = 1) otherwise;
//   * the DOUBLE COVER has the nodes 2 f + bit; a pair (f, g, s) joins 2 f with 2 g + s and 2 f + 1 with 2 g + (1 - s), by
//     cc_union of meshcc.hpp unchanged on a parent array of 2 F ints (parent[x] <= x, atomicMin only).  root(2 f) >> 1 is the
//     lowest face of f's orientation component, root(2 f) == root(2 f + 1) marks a non-orientable component, and otherwise
//     b(f) = root(2 f) & 1 is the flip of f relative to that lowest face;
//   * the sign policies sum det(q0, q1, q2) of the quantised corners in integers: |q| <= 2^18, so |det| < 2^57 is exact in int64,
//     and the low 32 bits and the arithmetic high part are accumulated apart, so that the sum of 2^28 faces cannot overflow;
//   * a BOUNDARY half-edge is a directed edge a->b of a valid face whose undirected edge carries exactly one valid face; a LOOP
//     is a connected component of them through shared vertex ids (cc_union over the vertices), SIMPLE when every vertex on it
//     has one outgoing and one incoming boundary half-edge;
//   * a filled loop gets one vertex at the fixed-point mean of its vertices (the rule and constants of meshsimp.hpp) and one
//     face (b, a, c) per half-edge a->b.
//
// arah_mesh_orient, one launch per line:
//
//   k_mo_init        parent[i] = i for the 2 F nodes, the per-component tables and counts cleared
//   k_mo_pairs       one thread per (face, corner): the entry (a, b) of nbr by bisection, nbr_out + nbr_in == 2, the shorter of
//                    the two vf segments scanned for the other face that names both ends; the two unions from the lower face id
//   k_mo_flatten     froot[f] = root(2 f) >> 1 (or -1), fstate[f] = b | non-orientable << 1; read-only on parent
//   k_cc_compact<kCcRoots>, k_mc_scan, k_cc_compact<kCcRoots>   components numbered in ascending order of their lowest face
//   k_mo_label       face_comp, comp_faces, the faces with b = 1 per component, bit 0 of comp_flags (by the lowest face alone)
//   k_mo_volume      (sign policies) the split integer volume of every component as the seed orients it
//   k_mo_decide      one thread per component: the policy -> bit 1 of comp_flags
//   k_mo_apply       flip, faces_out
//
// arah_mesh_boundary_loops: k_mo_loop_init, k_mo_compact<kMoBoundary> (count, k_mc_scan, fill: edges, edge_face, the vertices'
// boundary degrees, the unions), k_mo_loop_flatten, k_cc_compact<kCcRoots> (count, k_mc_scan, fill), k_mo_loop_verts,
// k_mo_loop_edges, k_mo_loop_finish.  arah_mesh_fill_holes: k_mo_fill_init, k_mo_fill_accum, k_mo_compact<kMoLoops>,
// k_mo_compact<kMoFilled> (count, k_mc_scan, fill each), k_mo_fill_copy, k_mc_pad_words.
//
// Integer atomics only (min, add, or): minima, sums and disjunctions of integers do not depend on the order of arrival.  No
// thread waits for another: no spin-wait, no grid-wide barrier; every loop ends by an argument of its own, stated at the loop.
// The adjacency, the edges and the loop tables are the CALLER's arrays: no value read from them is followed out of bounds.
// The constants, mesh_compact (the walk of k_mo_compact), k_mc_scan, k_mc_pad_words and cc_add_one are meshcommon.hpp's; the
// clamped segment (ma_segment) is meshedge.hpp's.
#pragma once

constexpr double kMoVolLimit = 262144.0;  // 2^18: three such factors and six terms stay below 2^57
enum { kMoSeed = 0, kMoMajority = 1, kMoNegative = 2, kMoPositive = 3 };

struct MoQuant {
    float origin[3];
    double scale;
};

// number of valid faces on the undirected edge {a, b}: the entry (a, b) of the sorted neighbour CSR by bisection, 0 when absent.
// The adjacency is the caller's: ma_find's unclamped segment is not for it, the rows are clamped first (ma_segment); the loop
// leaves at the first equal row, which ma_find's lower bound does not
__device__ __forceinline__ int mo_edge_faces(const int* __restrict__ nbr_start, const int* __restrict__ nbr,
                                             const int* __restrict__ nbr_out, const int* __restrict__ nbr_in, long long rows, int a, int b) {
    long long lo, hi;
    ma_segment(nbr_start, a, rows, lo, hi);
    while (lo < hi) {   // terminates: hi - lo strictly decreases (lo < mid + 1 <= hi or hi = mid < hi)
        const long long mid = lo + ((hi - lo) >> 1);
        const int n = nbr[mid];
        if (n == b) return nbr_out[mid] + nbr_in[mid];
        if (n < b) lo = mid + 1; else hi = mid;
    }
    return 0;
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_init(int* __restrict__ parent, int n_faces, int* __restrict__ comp_faces,
                                                           int* __restrict__ comp_flags, int* __restrict__ comp_ones,
                                                           long long* __restrict__ vol_hi, long long* __restrict__ vol_lo,
                                                           int* __restrict__ counts) {
    const long long step = (long long)gridDim.x * blockDim.x, n = 2 * (long long)n_faces;
    // terminates: n - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        parent[i] = (int)i;
        if (i < n_faces) {
            comp_faces[i] = 0;
            comp_flags[i] = 0;
            comp_ones[i] = 0;
            vol_hi[i] = 0;
            vol_lo[i] = 0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_pairs(const int* __restrict__ faces, int n_faces, int n_verts,
                                                            const int* __restrict__ vf_start, const int* __restrict__ vf,
                                                            const int* __restrict__ nbr_start, const int* __restrict__ nbr,
                                                            const int* __restrict__ nbr_out, const int* __restrict__ nbr_in, int* parent) {
    const long long step = (long long)gridDim.x * blockDim.x, n = 3 * (long long)n_faces;
    // terminates: n - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const int f = (int)(i / 3), c = (int)(i - 3 * (long long)f);
        int id[3];
        if (!ma_face_ok(faces, f, n_verts, id)) continue;
        const int a = id[c], b = id[(c + 1) % 3];
        if (mo_edge_faces(nbr_start, nbr, nbr_out, nbr_in, 6 * (long long)n_faces, a, b) != 2) continue;
        long long alo, ahi, blo, bhi;
        ma_segment(vf_start, a, 3 * (long long)n_faces, alo, ahi);
        ma_segment(vf_start, b, 3 * (long long)n_faces, blo, bhi);
        const bool by_a = ahi - alo <= bhi - blo;
        const long long last = by_a ? ahi : bhi;
        const int other = by_a ? b : a;
        for (long long j = by_a ? alo : blo; j < last; ++j) {   // terminates: last - j strictly decreases
            const int g = vf[j];
            int gd[3];
            if (g == f || (unsigned)g >= (unsigned)n_faces || !ma_face_ok(faces, g, n_verts, gd)) continue;
            if (gd[0] != other && gd[1] != other && gd[2] != other) continue;
            const int ka = gd[0] == a ? 0 : gd[1] == a ? 1 : gd[2] == a ? 2 : -1;
            if (ka < 0) continue;   // a face of the scanned segment names its vertex; a caller's array may not
            // exactly two valid faces lie on the edge: g is THE partner; the lower face id joins the pair
            if (f < g) {
                const int s = gd[(ka + 1) % 3] == b ? 1 : 0;   // g traverses a->b as f does: inconsistent
                cc_union(parent, 2 * f, 2 * g + s);
                cc_union(parent, 2 * f + 1, 2 * g + (1 - s));
            }
            break;
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_flatten(const int* __restrict__ faces, int n_faces, int n_verts,
                                                              const int* __restrict__ parent, int* __restrict__ froot,
                                                              unsigned char* __restrict__ fstate) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_faces - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += step) {
        int id[3];
        if (!ma_face_ok(faces, f, n_verts, id)) {
            froot[f] = -1;
            fstate[f] = 0;
            continue;
        }
        const int r0 = cc_walk(parent, 2 * (int)f), r1 = cc_walk(parent, 2 * (int)f + 1);   // parent is final: the launch boundary
        froot[f] = r0 >> 1;
        fstate[f] = (unsigned char)(r0 == r1 ? 2 : (r0 & 1));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_label(const int* __restrict__ froot, const unsigned char* __restrict__ fstate,
                                                            const int* __restrict__ dense, int n_faces, int* __restrict__ face_comp,
                                                            int* comp_faces, int* comp_ones, int* __restrict__ comp_flags, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0; the face count is rounded up to
    // whole waves so that every lane reaches cc_add_one and the ballots
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        const int r = f < n_faces ? froot[f] : -1;
        const bool ok = r >= 0;
        const int c = ok ? dense[r] : 0;   // r < n_faces is the lowest face of a component: k_cc_compact numbered it
        const int st = ok ? fstate[f] : 0;
        if (f < n_faces) face_comp[f] = ok ? c : -1;
        cc_add_one(comp_faces, c, ok);
        cc_add_one(comp_ones, c, ok && st == 1);
        if (ok && r == (int)f && st == 2) comp_flags[c] = 1;   // one writer: the component's lowest face
        const unsigned long long valid = __ballot(ok), ones = __ballot(ok && st == 1);
        if (lane == 0 && valid) atomicAdd(&counts[0], (int)__popcll(valid));
        if (lane == 0 && ones) atomicAdd(&counts[3], (int)__popcll(ones));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_volume(const float* __restrict__ verts, const int* __restrict__ faces, int n_faces,
                                                             int n_verts, MoQuant g, const int* __restrict__ face_comp,
                                                             const unsigned char* __restrict__ fstate, long long* vol_hi, long long* vol_lo) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0; the face count is rounded up to
    // whole waves so that every lane reaches the ballots and the shuffles
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        int c = -1, id[3];
        bool active = f < n_faces;
        if (active) {
            c = face_comp[f];
            active = c >= 0 && ma_face_ok(faces, f, n_verts, id);
        }
        long long d = 0;
        if (active) {
            long long q[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float x = verts[3 * (size_t)id[k] + a];
                    active = active && isfinite(x);
                    const double t = ((double)x - (double)g.origin[a]) * g.scale;
                    q[k][a] = active ? llrint(fmin(fmax(t, -kMoVolLimit), kMoVolLimit)) : 0;
                }
            d = q[0][0] * (q[1][1] * q[2][2] - q[1][2] * q[2][1]) - q[0][1] * (q[1][0] * q[2][2] - q[1][2] * q[2][0]) +
                q[0][2] * (q[1][0] * q[2][1] - q[1][1] * q[2][0]);
            if (fstate[f] == 1) d = -d;
        }
        // two's complement: the unsigned sums are the signed ones.  Integer sums do not depend on how they are grouped, so a wave
        // whose faces all belong to one component (a body mesh has one) adds them up first and issues two atomics, not 128
        unsigned long long lo = active ? (unsigned long long)d & 0xFFFFFFFFull : 0ull, hi = active ? (unsigned long long)(d >> 32) : 0ull;
        const unsigned long long pending = __ballot(active);
        if (!pending) continue;   // the same for every lane of the wave
        const int c0 = __shfl(c, __ffsll((long long)pending) - 1);
        if (__ballot(active && c != c0) == 0ull) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo += __shfl_down(lo, o);
                hi += __shfl_down(hi, o);
            }
            if (lane == 0) {
                atomicAdd(reinterpret_cast<unsigned long long*>(&vol_lo[c0]), lo);
                atomicAdd(reinterpret_cast<unsigned long long*>(&vol_hi[c0]), hi);
            }
        } else if (active) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&vol_lo[c]), lo);
            atomicAdd(reinterpret_cast<unsigned long long*>(&vol_hi[c]), hi);
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_decide(const int* __restrict__ comp_faces, const int* __restrict__ comp_ones,
                                                             const long long* __restrict__ vol_hi, const long long* __restrict__ vol_lo,
                                                             int policy, int* __restrict__ comp_flags, int* counts) {
    const int n_comp = counts[1];
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_comp + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    // terminates: end - c strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < end; c += step) {
        bool nonor = false, rev = false;
        if (c < n_comp) {
            nonor = (comp_flags[c] & 1) != 0;
            const int ones = comp_ones[c];
            const bool majority = ones > comp_faces[c] - ones;
            // hi 2^32 + lo with lo in [0, 2^60): the carry of lo goes to hi, what is left of lo is below 2^32 and cannot outweigh it
            const long long hi = vol_hi[c] + (vol_lo[c] >> 32), lo = vol_lo[c] & 0xFFFFFFFFll;
            const int sign = hi > 0 ? 1 : hi < 0 ? -1 : lo > 0 ? 1 : 0;
            if (policy == kMoMajority) rev = majority;
            if (policy == kMoNegative) rev = sign == 0 ? majority : sign > 0;
            if (policy == kMoPositive) rev = sign == 0 ? majority : sign < 0;
            rev = rev && !nonor;
            if (rev) comp_flags[c] |= 2;
        }
        const unsigned long long n_nonor = __ballot(nonor), n_rev = __ballot(rev);
        if (lane == 0 && n_nonor) atomicAdd(&counts[2], (int)__popcll(n_nonor));
        if (lane == 0 && n_rev) atomicAdd(&counts[4], (int)__popcll(n_rev));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_apply(const int* __restrict__ faces, int n_faces, const int* __restrict__ face_comp,
                                                            const unsigned char* __restrict__ fstate, const int* __restrict__ comp_flags,
                                                            unsigned char* __restrict__ flip, int* __restrict__ faces_out, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        bool fl = false;
        if (f < n_faces) {
            const int c = face_comp[f];
            if (c >= 0) {
                const int flags = comp_flags[c];
                fl = !(flags & 1) && (((int)fstate[f] ^ (flags >> 1)) & 1);
            }
            const int a = faces[3 * f + 0], b = faces[3 * f + 1], d = faces[3 * f + 2];
            flip[f] = fl ? 1 : 0;
            faces_out[3 * f + 0] = a;
            faces_out[3 * f + 1] = fl ? d : b;
            faces_out[3 * f + 2] = fl ? b : d;
        }
        const unsigned long long n_fl = __ballot(fl);
        if ((threadIdx.x & 63) == 0 && n_fl) atomicAdd(&counts[5], (int)__popcll(n_fl));
    }
}

// ---- boundary loops ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mo_loop_init(int* __restrict__ parent, int* __restrict__ vout, int* __restrict__ vin,
                                                                int* __restrict__ bad, int n_verts, int* __restrict__ loop_edges,
                                                                unsigned char* __restrict__ loop_simple, int* __restrict__ loop_vert,
                                                                int* __restrict__ counts) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        parent[v] = (int)v;
        vout[v] = 0;
        vin[v] = 0;
        bad[v] = 0;
        loop_edges[v] = 0;
        loop_simple[v] = 0;
        loop_vert[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) counts[threadIdx.x] = 0;
}

// mesh_compact (meshcommon.hpp) over n elements, or over *n_dev clamped to [0, n] when n_dev is given.
//   WHAT          element, mark                                                   fill
//   kMoBoundary   (face, corner) i: the face is valid and one face lies on its    edges[id] = (a, b), edge_face[id] = face; the
//                 edge a->b                                                       boundary degrees of a and b; union(a, b)
//   kMoLoops      loop l: simple, 3 <= loop_edges <= max_edges, no non-finite     lrank[l] = id or -1; the new vertex V + id and its
//                 vertex                                                          source
//   kMoFilled     boundary edge e: its loop is filled                             the new face F + id and its loop
enum { kMoBoundary = 0, kMoLoops = 1, kMoFilled = 2 };

struct MoCompact {
    const int* faces; int n_faces; int n_verts;
    const int* nbr_start; const int* nbr; const int* nbr_out; const int* nbr_in;              // kMoBoundary
    int* edges; int* edge_face; int* vout; int* vin; int* parent;
    const int* loop_edges; const unsigned char* loop_simple; const int* loop_vert;            // kMoLoops
    const int* nonfinite; const long long* sums; int max_edges; MoQuant g;
    int* lrank; float* verts_out; int* vert_src;
    const int* edges_in; const int* edge_loop; int n_loops_cap;                               // kMoFilled
    int* faces_out; int* face_loop;
};

struct MoElement {
    int a, b;   // kMoBoundary: the half-edge a->b
    int of;     // kMoBoundary: its face; kMoFilled: its loop
};

template <int WHAT, bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_mo_compact(MoCompact p, int n, const int* __restrict__ n_dev, int* __restrict__ blk_count,
                                                              const int* __restrict__ blk_base) {
    const long long count = n_dev ? min(max((long long)*n_dev, 0ll), (long long)n) : (long long)n;
    mesh_compact<FILL, MoElement>(
        count, blk_count, blk_base,
        [&](long long i, MoElement& e) {
            if constexpr (WHAT == kMoBoundary) {
                const int f = (int)(i / 3), c = (int)(i - 3 * (long long)f);
                int id[3];
                if (!ma_face_ok(p.faces, f, p.n_verts, id)) return false;
                e.a = id[c];
                e.b = id[(c + 1) % 3];
                e.of = f;
                return mo_edge_faces(p.nbr_start, p.nbr, p.nbr_out, p.nbr_in, 6 * (long long)p.n_faces, e.a, e.b) == 1;
            }
            if constexpr (WHAT == kMoLoops) {
                const int m = p.loop_edges[i];
                return p.loop_simple[i] != 0 && m >= 3 && m <= p.max_edges && p.nonfinite[i] == 0;
            }
            if constexpr (WHAT == kMoFilled) {
                e.of = p.edge_loop[i];
                return (unsigned)e.of < (unsigned)p.n_loops_cap && p.lrank[e.of] >= 0;
            }
        },
        [&](long long i, bool ok, bool mark, int id, const MoElement& e) {
#pragma clang fp contract(off)
            const long long at = id;
            if constexpr (WHAT == kMoBoundary) {
                if (mark) {   // at < the marks in all <= 3 F: the rows of edges and edge_face
                    p.edges[2 * at + 0] = e.a;
                    p.edges[2 * at + 1] = e.b;
                    p.edge_face[at] = e.of;
                    atomicAdd(&p.vout[e.a], 1);
                    atomicAdd(&p.vin[e.b], 1);
                    cc_union(p.parent, e.a, e.b);
                }
            }
            if constexpr (WHAT == kMoLoops) {
                if (ok) p.lrank[i] = mark ? (int)at : -1;
                // a filled loop has at least 3 vertices of its own, so at < V / 3, the rows behind the first V; the test keeps a
                // caller's table that claims more loops than that inside the array
                if (mark && at < p.n_verts / 3) {
                    const long long row = (long long)p.n_verts + at;
                    const double m = (double)p.loop_edges[i];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        p.verts_out[3 * row + a] = (float)((double)p.g.origin[a] + ((double)p.sums[3 * i + a] / m) / p.g.scale);
                    p.vert_src[row] = p.loop_vert[i];
                }
            }
            if constexpr (WHAT == kMoFilled) {
                if (mark) {   // at < the boundary edges <= 3 F: the rows behind the first F
                    const long long row = (long long)p.n_faces + at;
                    p.faces_out[3 * row + 0] = p.edges_in[2 * i + 1];
                    p.faces_out[3 * row + 1] = p.edges_in[2 * i + 0];
                    p.faces_out[3 * row + 2] = p.n_verts + p.lrank[e.of];
                    p.face_loop[row] = e.of;
                }
            }
        });
}

// root[v] = the smallest vertex of v's loop for a vertex on a boundary half-edge, -1 for every other one: the marks root[v] == v
// of k_cc_compact<kCcRoots> are then the loops' smallest vertices.  Read-only on parent (the launch boundary made it final).
__global__ __launch_bounds__(kImeshThreads) void k_mo_loop_flatten(const int* __restrict__ parent, const int* __restrict__ vout,
                                                                   const int* __restrict__ vin, int n_verts, int* __restrict__ root) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step)
        root[v] = vout[v] + vin[v] > 0 ? cc_walk(parent, (int)v) : -1;
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_loop_verts(const int* __restrict__ root, const int* __restrict__ dense,
                                                                 const int* __restrict__ vout, const int* __restrict__ vin, int n_verts,
                                                                 int* __restrict__ loop_vert, int* bad) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const int r = root[v];
        if (r < 0) continue;
        const int l = dense[r];
        if (r == (int)v) loop_vert[l] = (int)v;   // one writer: the loop's smallest vertex
        if (vout[v] != 1 || vin[v] != 1) atomicOr(&bad[l], 1);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_loop_edges(const int* __restrict__ edges, int cap, const int* __restrict__ root,
                                                                 const int* __restrict__ dense, const int* __restrict__ counts,
                                                                 int* __restrict__ edge_loop, int* loop_edges) {
    const int n_edges = min(max(counts[0], 0), cap);
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_edges + 63) & ~63ll;
    // terminates: end - e strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < end; e += step) {
        const bool ok = e < n_edges;
        const int l = ok ? dense[root[edges[2 * e]]] : 0;   // edges[] was written by this call: a vertex with vout > 0, root >= 0
        if (ok) edge_loop[e] = l;
        cc_add_one(loop_edges, l, ok);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_loop_finish(const int* __restrict__ bad, int n_verts, unsigned char* __restrict__ loop_simple,
                                                                  int* counts) {
    const int n_loops = min(max(counts[1], 0), n_verts);
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_loops + 63) & ~63ll;
    // terminates: end - l strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long l = (long long)blockIdx.x * blockDim.x + threadIdx.x; l < end; l += step) {
        const bool simple = l < n_loops && bad[l] == 0;
        if (l < n_loops) loop_simple[l] = simple ? 1 : 0;
        const unsigned long long n_simple = __ballot(simple);
        if ((threadIdx.x & 63) == 0 && n_simple) atomicAdd(&counts[2], (int)__popcll(n_simple));
    }
}

// ---- hole filling --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kImeshThreads) void k_mo_fill_init(long long* __restrict__ sums, int* __restrict__ nonfinite, int n_verts,
                                                                const int* __restrict__ loop_counts, int* __restrict__ counts) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        sums[3 * v + 0] = 0;
        sums[3 * v + 1] = 0;
        sums[3 * v + 2] = 0;
        nonfinite[v] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 5) counts[threadIdx.x] = threadIdx.x < 3 ? loop_counts[threadIdx.x] : 0;
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_fill_accum(const float* __restrict__ verts, int n_verts, const int* __restrict__ edges,
                                                                 const int* __restrict__ edge_loop, int cap, const int* __restrict__ loop_counts,
                                                                 const int* __restrict__ loop_edges, const unsigned char* __restrict__ loop_simple,
                                                                 int max_edges, MoQuant g, long long* sums, int* nonfinite) {
#pragma clang fp contract(off)
    const int n_edges = min(max(loop_counts[0], 0), cap);
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_edges - e strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += step) {
        const int l = edge_loop[e], a = edges[2 * e];
        if ((unsigned)l >= (unsigned)n_verts || (unsigned)a >= (unsigned)n_verts) continue;   // the caller's arrays
        const int m = loop_edges[l];
        if (!loop_simple[l] || m < 3 || m > max_edges) continue;
        // a simple loop: every vertex on it starts exactly one half-edge, so the starts are the loop's vertices, each once
        const float x[3] = {verts[3 * (size_t)a + 0], verts[3 * (size_t)a + 1], verts[3 * (size_t)a + 2]};
        if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) {
            atomicOr(&nonfinite[l], 1);
            continue;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double t = ((double)x[k] - (double)g.origin[k]) * g.scale;
            const long long q = llrint(fmin(fmax(t, -kMsFixLimit), kMsFixLimit));
            // two's complement: the unsigned sum is the signed one
            atomicAdd(reinterpret_cast<unsigned long long*>(&sums[3 * (size_t)l + k]), (unsigned long long)q);
        }
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_mo_fill_copy(const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                                                int n_faces, float* __restrict__ verts_out, int* __restrict__ vert_src,
                                                                int* __restrict__ faces_out, int* __restrict__ face_loop) {
    const long long step = (long long)gridDim.x * blockDim.x, n = max((long long)n_verts, (long long)n_faces);
    // terminates: n - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        if (i < n_verts) {
            verts_out[3 * i + 0] = verts[3 * i + 0];
            verts_out[3 * i + 1] = verts[3 * i + 1];
            verts_out[3 * i + 2] = verts[3 * i + 2];
            vert_src[i] = (int)i;
        }
        if (i < n_faces) {
            faces_out[3 * i + 0] = faces[3 * i + 0];
            faces_out[3 * i + 1] = faces[3 * i + 1];
            faces_out[3 * i + 2] = faces[3 * i + 2];
            face_loop[i] = -1;
        }
    }
}

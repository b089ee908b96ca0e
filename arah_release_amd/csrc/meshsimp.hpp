// meshsimp.hpp -- simplification of an indexed mesh by vertex clustering on a grid, on the device.
//
// Reference: none.  The reference writes the mesh skimage extracts as it comes (utils/sdf_meshing.py:95-114): marching cubes
// tessellates the body uniformly, whatever the curvature.  Here the vertices that fall into one cell of a caller's grid become
// ONE vertex, faces are renamed to cells, and the faces that collapse or repeat go: decimation and welding by position.  Every
// decision is an integer one, so the result is unique and is compared bit for bit with the tensor specification
// (meshing.mesh_simplify), like meshcc.hpp:
//
//   * cell of a vertex: c = clamp(floor((v - origin) inv_cell), 0, dims - 1) per axis in float32 -- one subtraction, one
//     multiplication, nothing to contract; key = cx + nx (cy + ny cz); a vertex with a non-finite coordinate has no cell;
//   * clusters = occupied cells, numbered in ascending key: the rank of the cell's bit in a bitmap;
//   * position: q = llrint(clamp((double(v) - double(origin)) scale, -2^36, 2^36)), scale a power of two the host chose so that
//     a vertex inside the grid has q in [0, 2^36]; S = sum q, n = count by INTEGER atomics (at most 2^26 vertices: |S| <= 2^62);
//     mean = float32(double(origin) + (double(S) / double(n)) / scale) -- the division by a power of two is exact, so a fused
//     and an unfused evaluation of the line agree;
//   * representative: the member with the smallest d^2 = float32((dx dx + dy dy) + dz dz), d = double(v) - double(mean),
//     contraction off; ties to the lowest id: one 64-bit atomicMin of (bits(d^2) << 32) | id;
//   * a face with an id outside [0, V) or an invalid vertex is dropped (counts[2]); a face two of whose three clusters are equal
//     is collapsed (counts[3]); with dedup a face is a duplicate (counts[4]) when an earlier surviving face names the same three
//     clusters: a 64-bit open-addressing table keyed by the three sorted 21-bit ids holds the lowest row of every key.
//
// arah_mesh_simplify, one launch per line:
//
//   k_ms_init      bitmap, sums, counts of members, packed minima, the table, the face counters: cleared
//   k_ms_mark      one thread per vertex: vkey[v] = its key or -1, atomicOr of the cell's bit (as tier.hpp marks voxels)
//   k_ms_popc      wcount[w] = popcount(bitmap[w])
//   k_mc_scan      wbase = their exclusive scan, counts[0] = K.  Cluster of a key = wbase[key / 32] + the bits below it in its word
//   k_ms_accum     vert_map[v] = the cluster; S[cluster] += q, n[cluster] += 1
//   k_ms_pick      best[cluster] = min over members of (bits(d^2) << 32) | v
//   k_ms_finish    per cluster: vert_src, verts_out (mean or member); rows from K on zeroed; the status (dedup and K > 2^21)
//   k_ms_classify  one thread per face: invalid / collapsed / survivor; a survivor claims the slot of its key (atomicCAS on the
//                  key, probing linearly) and atomicMin's its row into the slot; fslot[f] = the slot, or -1 for a face that goes
//   k_ms_compact<false>, k_mc_scan, k_ms_compact<true>
//                  the count / scan / fill of meshcommon.hpp over the mark "fslot[f] >= 0 and the slot's row is f": kept faces in
//                  their original order and orientation, face_src; rows from the count on zeroed; counts[4] by subtraction
//
// Integer atomics only (or, add, min, compare-and-swap): none of the results depends on the order of arrival -- the table's
// LAYOUT does, but only "the lowest row of my key" is ever read from it.  No thread waits for another: no spin-wait, no
// grid-wide barrier; every loop ends by an argument of its own, stated at the loop.
#pragma once

constexpr int kMsKeyBits = 21;            // bits of a cluster id inside a face's key
constexpr double kMsFixLimit = 68719476736.0;   // 2^36
constexpr unsigned long long kMsEmpty = ~0ull;   // no key: a key has 63 bits

struct MsGrid {
    float origin[3];
    float inv_cell;
    int dims[3];
    double scale;
};

// key of the cell of v, or -1 for a vertex with a non-finite coordinate
__device__ __forceinline__ int ms_key(const MsGrid& g, const float v[3]) {
#pragma clang fp contract(off)
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(v[a])) return -1;
        const float t = floorf((v[a] - g.origin[a]) * g.inv_cell);
        // 2^27 is a float32 and bounds every dims; dims - 1 itself need not be one, so the upper clamp is an integer's
        c[a] = min((int)fminf(fmaxf(t, 0.0f), 134217728.0f), g.dims[a] - 1);
    }
    return c[0] + g.dims[0] * (c[1] + g.dims[1] * c[2]);
}

__device__ __forceinline__ int ms_cluster(const unsigned* __restrict__ bitmap, const int* __restrict__ wbase, int key) {
    return wbase[key >> 5] + __popc(bitmap[key >> 5] & ((1u << (key & 31)) - 1u));
}

__device__ __forceinline__ float ms_mean(const MsGrid& g, const long long* __restrict__ S, const int* __restrict__ members, int k, int a) {
#pragma clang fp contract(off)
    return (float)((double)g.origin[a] + ((double)S[3 * (size_t)k + a] / (double)members[k]) / g.scale);
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_init(unsigned* __restrict__ bitmap, long long n_words, long long* __restrict__ S,
                                                           int* __restrict__ members, unsigned long long* __restrict__ best, int n_verts,
                                                           unsigned long long* __restrict__ tkeys, int* __restrict__ trows,
                                                           long long n_slots, int* __restrict__ counts) {
    const long long step = (long long)gridDim.x * blockDim.x;
    const long long end = max(max(n_words, (long long)n_verts), n_slots);
    // terminates: end - i strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += step) {
        if (i < n_words) bitmap[i] = 0u;
        if (i < n_verts) {
            S[3 * i + 0] = 0;
            S[3 * i + 1] = 0;
            S[3 * i + 2] = 0;
            members[i] = 0;
            best[i] = kMsEmpty;
        }
        if (i < n_slots) {
            tkeys[i] = kMsEmpty;
            trows[i] = 0x7FFFFFFF;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < 6) counts[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_mark(const float* __restrict__ verts, int n_verts, MsGrid g, int* __restrict__ vkey,
                                                           unsigned* bitmap) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const float p[3] = {verts[3 * v + 0], verts[3 * v + 1], verts[3 * v + 2]};
        const int key = ms_key(g, p);
        vkey[v] = key;
        if (key >= 0) atomicOr(&bitmap[key >> 5], 1u << (key & 31));
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_popc(const unsigned* __restrict__ bitmap, long long n_words, int* __restrict__ wcount) {
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_words - w strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long w = (long long)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += step) wcount[w] = __popc(bitmap[w]);
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_accum(const float* __restrict__ verts, int n_verts, MsGrid g,
                                                            const int* __restrict__ vkey, const unsigned* __restrict__ bitmap,
                                                            const int* __restrict__ wbase, int* __restrict__ vert_map, long long* S,
                                                            int* members) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const int key = vkey[v];
        if (key < 0) {
            vert_map[v] = -1;
            continue;
        }
        const int k = ms_cluster(bitmap, wbase, key);
        vert_map[v] = k;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = ((double)verts[3 * v + a] - (double)g.origin[a]) * g.scale;
            const long long q = llrint(fmin(fmax(x, -kMsFixLimit), kMsFixLimit));
            // two's complement: the unsigned sum is the signed one
            atomicAdd(reinterpret_cast<unsigned long long*>(&S[3 * (size_t)k + a]), (unsigned long long)q);
        }
        atomicAdd(&members[k], 1);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_pick(const float* __restrict__ verts, int n_verts, MsGrid g,
                                                           const int* __restrict__ vert_map, const long long* __restrict__ S,
                                                           const int* __restrict__ members, unsigned long long* best) {
#pragma clang fp contract(off)
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - v strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < n_verts; v += step) {
        const int k = vert_map[v];
        if (k < 0) continue;
        const double dx = (double)verts[3 * v + 0] - (double)ms_mean(g, S, members, k, 0);
        const double dy = (double)verts[3 * v + 1] - (double)ms_mean(g, S, members, k, 1);
        const double dz = (double)verts[3 * v + 2] - (double)ms_mean(g, S, members, k, 2);
        const float d2 = (float)((dx * dx + dy * dy) + dz * dz);
        // d2 >= +0: the bits of a non-negative float order like the float
        atomicMin(&best[k], ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)v);
    }
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_finish(const float* __restrict__ verts, int n_verts, MsGrid g, int use_member,
                                                             int dedup, const long long* __restrict__ S, const int* __restrict__ members,
                                                             const unsigned long long* __restrict__ best, int* counts,
                                                             float* __restrict__ verts_out, int* __restrict__ vert_src) {
    const int n_clusters = counts[0];
    // the status: three cluster ids of more than kMsKeyBits bits do not fit a face's key
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[5] = dedup && n_clusters > (1 << kMsKeyBits) ? 1 : 0;
    const long long step = (long long)gridDim.x * blockDim.x;
    // terminates: n_verts - k strictly decreases (step >= 1) and the loop ends when it reaches 0
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n_verts; k += step) {
        int src = 0;
        float p[3] = {0.f, 0.f, 0.f};
        if (k < n_clusters) {   // a cluster has a member, and the member an id below n_verts
            src = (int)(best[k] & 0xFFFFFFFFull);
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = use_member ? verts[3 * (size_t)src + a] : ms_mean(g, S, members, (int)k, a);
        }
        vert_src[k] = src;
        verts_out[3 * k + 0] = p[0];
        verts_out[3 * k + 1] = p[1];
        verts_out[3 * k + 2] = p[2];
    }
}

// splitmix64's finaliser: the slot a key starts probing at
__device__ __forceinline__ unsigned long long ms_hash(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(kImeshThreads) void k_ms_classify(const int* __restrict__ faces, int n_faces, int n_verts,
                                                               const int* __restrict__ vert_map, int dedup,
                                                               unsigned long long* tkeys, int* trows, long long n_slots,
                                                               int* __restrict__ fslot, int* counts) {
    const long long step = (long long)gridDim.x * blockDim.x, end = ((long long)n_faces + 63) & ~63ll;
    const int lane = threadIdx.x & 63;
    const bool too_many = counts[5] != 0;   // k_ms_finish set it: no face is kept
    // terminates: end - f strictly decreases (step >= 1) and the loop ends when it reaches 0.  The face count is rounded up to
    // whole waves so that every lane reaches the ballots; lanes beyond the end carry no face
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < end; f += step) {
        int id[3] = {0, 0, 0};
        const bool in_face = f < n_faces;
        bool ok = in_face && cc_face_ok(faces, f, n_verts, id);
        int c[3] = {-1, -1, -1};
        if (ok) {
            c[0] = vert_map[id[0]];
            c[1] = vert_map[id[1]];
            c[2] = vert_map[id[2]];
            ok = c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
        }
        const bool invalid = in_face && !ok;
        const bool collapsed = ok && (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]);
        int slot = -1;
        if (ok && !collapsed && !too_many) {
            slot = 0;
            if (dedup) {
                const int lo = min(c[0], min(c[1], c[2])), hi = max(c[0], max(c[1], c[2])), mid = c[0] + c[1] + c[2] - lo - hi;
                const unsigned long long key = (unsigned long long)lo | ((unsigned long long)mid << kMsKeyBits) |
                                               ((unsigned long long)hi << (2 * kMsKeyBits));
                long long s = (long long)(ms_hash(key) & (unsigned long long)(n_slots - 1));
                slot = -1;
                // terminates: at most n_slots probes, each at another slot.  It ends EARLIER, at an empty slot or at the key's own:
                // the table has at least 2 n_faces slots and a face claims at most one, so empty slots never run out.  A probe
                // is one compare-and-swap whose answer is final (a claimed slot keeps its key for good): nothing is retried
                for (long long probe = 0; probe < n_slots; ++probe) {
                    const unsigned long long old = atomicCAS(&tkeys[s], kMsEmpty, key);
                    if (old == kMsEmpty || old == key) {
                        atomicMin(&trows[s], (int)f);
                        slot = (int)s;
                        break;
                    }
                    s = (s + 1) & (n_slots - 1);
                }
            }
        }
        if (in_face) fslot[f] = slot;
        const unsigned long long n_inv = __ballot(invalid), n_col = __ballot(collapsed);
        if (lane == 0 && n_inv) atomicAdd(&counts[2], (int)__popcll(n_inv));
        if (lane == 0 && n_col) atomicAdd(&counts[3], (int)__popcll(n_col));
    }
}

// mesh_compact (meshcommon.hpp) over the faces; a face is kept when it claimed a slot and, with dedup, its row is the slot's
// minimum.  FILL also zeroes the rows from the kept count on (counts[1], final since the scan) and derives the duplicates: what is
// neither invalid, collapsed nor kept -- nothing when the status is set.
template <bool FILL>
__global__ __launch_bounds__(kImeshThreads) void k_ms_compact(const int* __restrict__ faces, int n_faces, const int* __restrict__ vert_map,
                                                              const int* __restrict__ fslot, const int* __restrict__ trows, int dedup,
                                                              int* __restrict__ blk_count, const int* __restrict__ blk_base,
                                                              int* __restrict__ faces_out, int* __restrict__ face_src, int* counts) {
    const int kept = FILL ? counts[1] : 0;
    mesh_compact<FILL, MeshNoState>(
        n_faces, blk_count, blk_base,
        [&](long long i, MeshNoState&) {
            const int slot = fslot[i];
            return slot >= 0 && (!dedup || trows[slot] == (int)i);
        },
        [&](long long i, bool ok, bool mark, int at, const MeshNoState&) {
            if (mark) {   // at < kept <= n_faces
                faces_out[3 * (long long)at + 0] = vert_map[faces[3 * i + 0]];
                faces_out[3 * (long long)at + 1] = vert_map[faces[3 * i + 1]];
                faces_out[3 * (long long)at + 2] = vert_map[faces[3 * i + 2]];
                face_src[at] = (int)i;
            }
            if (ok && i >= kept) {   // rows below `kept` are written by the faces that land there, the others here
                faces_out[3 * i + 0] = 0;
                faces_out[3 * i + 1] = 0;
                faces_out[3 * i + 2] = 0;
                face_src[i] = 0;
            }
        });
    if (FILL && blockIdx.x == 0 && threadIdx.x == 0) counts[4] = counts[5] ? 0 : n_faces - counts[2] - counts[3] - kept;
}

// a mesh without a vertex: no cluster, every face invalid
__global__ void k_ms_set_empty(int* __restrict__ counts, int n_faces) {
    if (blockIdx.x == 0 && threadIdx.x < 6) counts[threadIdx.x] = threadIdx.x == 2 ? n_faces : 0;
}

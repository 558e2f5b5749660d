// Two-level Infomap on a kNN graph, entirely on the device: the pseudo-labelling step `cluster_by_infomap` of
// CC/clustercontrast/utils/infomap_cluster.py:129-227 between get_dist_nbr and generate_cluster_features.  Not the `infomap`
// package's seeded search but its objective (the two-level map equation on the flow of a directed graph, teleportation to
// links, unrecorded) under a deterministic search; the definition is DESIGN §6 and tests/infomap_hostmodel.py:
//   links     row i of the kNN table left to right: self entries skipped, an entry with dist <= thr is the link i -> nbr with
//             weight double(1.0f - dist), the first other entry ends the row;
//   flow      PageRank in fp64 (alpha 0.15, teleportation proportional to in-link weight, dangling nodes teleport with
//             probability 1) to an L1 change <= 1e-13, then link flow p_i w_ij / w_i normalised and node flow = in-flow;
//   L         plogp(sum enter) - sum plogp(enter) - sum plogp(exit) + sum plogp(exit + p) - sum_nodes plogp(p_node);
//   search    synchronous local-move sweeps over units (leaves, then aggregated modules), at most one admitted move per module
//             and sweep, driven from the host (rg_hip/ops/infomap.py: infomap_search).
// Everything works on CSR lists.  All flow and codelength arithmetic is fp64 and every sum runs in a fixed order (a thread
// walks its list front to back, a workgroup reduces in a fixed tree); the only atomics are integer ones whose result does
// not depend on the order they land in, so two runs give the same bits.  No kernel waits on another workgroup and every
// data-dependent loop is the host's.
#include "rg_common.h"
#include <limits.h>

namespace {

constexpr int kMaxN = 65536;
constexpr int kMaxK = 128;
constexpr int kRowsPerBlock = 4;          // one wavefront per kNN row / per unit
constexpr int kRed = 1024;                // threads of the single-workgroup reductions
constexpr double kAlpha = 0.15;           // teleportation probability
constexpr double kFlowTol = 1e-13;        // L1 change that ends the power iteration
constexpr double kMinGain = 1e-10;        // bits a move has to gain

// scal[] of the flow stage (fp64 device scalars)
enum { S_W = 0, S_NG = 1, S_ND = 2, S_DG = 3, S_DIFF = 4, S_ITERS = 5, S_DONE = 6, S_NODETERM = 7, S_Q = 8, S_COUNT = 16 };

__device__ __forceinline__ double plogp(double x) { return x > 0.0 ? x * log2(x) : 0.0; }

// sum over the workgroup of kRed threads in a fixed tree; every thread gets it
__device__ __forceinline__ double block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kRed / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------- links
// One wavefront walks row i, 64 entries per step.  The first entry that is neither self nor a link ends the row: a ballot of
// the failing entries and a find-first, no loop over the entries.  A neighbour index outside [0, N) counts as failing.
// FILL == false: cnt[i] = links of the row.  FILL == true: src / dst / w at rowptr[i] .., single[i], incnt[dst] += 1.
template <bool FILL>
__global__ __launch_bounds__(256) void infomap_links_kernel(const int* __restrict__ nbrs, const float* __restrict__ dists, int N, int k,
                                                            float thr, int* __restrict__ cnt, const int* __restrict__ rowptr,
                                                            int* __restrict__ src, int* __restrict__ dst, double* __restrict__ w,
                                                            int* __restrict__ single, int* __restrict__ incnt) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (i >= N) return;                   // whole wavefronts leave: the ballots below stay full
    const unsigned long long below = (1ull << lane) - 1ull;
    int pos = 0, end = 0, total = 0;
    if (FILL) {
        pos = rowptr[i];
        end = rowptr[i + 1];
    }
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int j = c0 + lane;
        const bool valid = j < k;
        const int nb = valid ? nbrs[(int64_t)i * k + j] : i;
        const float d = valid ? dists[(int64_t)i * k + j] : 0.f;
        const bool self = nb == i;
        const bool ok = valid && !self && (unsigned)nb < (unsigned)N && d <= thr;
        const bool fail = valid && !self && !ok;
        const unsigned long long fb = __ballot(fail);
        const unsigned long long before = fb ? ((1ull << (__ffsll((long long)fb) - 1)) - 1ull) : ~0ull;
        const bool link = ok && ((before >> lane) & 1ull);
        const unsigned long long lb = __ballot(link);
        if (FILL && link) {
            const int p = pos + __popcll(lb & below);
            if (p < end) {
                src[p] = i;
                dst[p] = nb;
                w[p] = (double)(1.0f - d);
                atomicAdd(incnt + nb, 1);
            }
        }
        pos += __popcll(lb);
        total += __popcll(lb);
        if (fb) break;                    // the same for every lane
    }
    if (lane == 0) {
        if (FILL)
            single[i] = total == 0;
        else
            cnt[i] = total;
    }
}

// ---------------------------------------------------------------------------------------------- flow
// wout[i] / win[i] = weight of the out / in links of node i, each list front to back
__global__ void infomap_weights_kernel(const int* __restrict__ orp, const double* __restrict__ w, const int* __restrict__ irp,
                                       const int* __restrict__ ieid, int N, double* __restrict__ wout, double* __restrict__ win) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double so = 0.0, si = 0.0;
    for (int e = orp[i]; e < orp[i + 1]; ++e) so += w[e];
    for (int e = irp[i]; e < irp[i + 1]; ++e) si += w[ieid[e]];
    wout[i] = so;
    win[i] = si;
}

// one workgroup: uniform p over the nodes that occur in a link, tele[j] = win[j] / total weight, the scalars of iteration 0
__global__ __launch_bounds__(kRed) void infomap_flow_start_kernel(const int* __restrict__ orp, const int* __restrict__ irp,
                                                                  const double* __restrict__ win, int N, double* __restrict__ p,
                                                                  double* __restrict__ tele, double* __restrict__ scal) {
    __shared__ double red[kRed];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < N; i += kRed) {
        a += win[i];
        b += (orp[i + 1] > orp[i] || irp[i + 1] > irp[i]) ? 1.0 : 0.0;
    }
    const double W = block_sum(a, red), ng = block_sum(b, red);
    double nd = 0.0, dg = 0.0;
    for (int i = threadIdx.x; i < N; i += kRed) {
        const bool out = orp[i + 1] > orp[i], in = irp[i + 1] > irp[i];
        const double pi = (out || in) ? 1.0 / ng : 0.0;
        p[i] = pi;
        tele[i] = win[i] / W;
        if (out)
            nd += pi;
        else
            dg += pi;
    }
    nd = block_sum(nd, red);
    dg = block_sum(dg, red);
    if (threadIdx.x == 0) {
        scal[S_W] = W;
        scal[S_NG] = ng;
        scal[S_ND] = nd;
        scal[S_DG] = dg;
        scal[S_DIFF] = 1.0;
        scal[S_ITERS] = 0.0;
        scal[S_DONE] = 0.0;
    }
}

// raw[j] = (1 - alpha) sum_i p_i w_ij / w_i (in-links in ascending source order) + (alpha nd + dg) tele[j]
__global__ void infomap_flow_pull_kernel(const int* __restrict__ irp, const int* __restrict__ isrc, const int* __restrict__ ieid,
                                         const double* __restrict__ w, const double* __restrict__ wout, const double* __restrict__ p,
                                         const double* __restrict__ tele, int N, const double* __restrict__ scal,
                                         double* __restrict__ raw) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N || scal[S_DONE] != 0.0) return;
    double s = 0.0;
    for (int e = irp[j]; e < irp[j + 1]; ++e) {
        const int i = isrc[e];
        s += p[i] * w[ieid[e]] / wout[i];
    }
    raw[j] = (1.0 - kAlpha) * s + (kAlpha * scal[S_ND] + scal[S_DG]) * tele[j];
}

// one workgroup: p = raw / sum raw, the L1 change and the two sums the next pull needs; sets the done flag
__global__ __launch_bounds__(kRed) void infomap_flow_update_kernel(const int* __restrict__ orp, const double* __restrict__ raw, int N,
                                                                   double* __restrict__ p, double* __restrict__ scal, int max_iters) {
    __shared__ double red[kRed];
    if (scal[S_DONE] != 0.0) return;      // written only after the barriers below: every thread reads the same value
    double z = 0.0;
    for (int i = threadIdx.x; i < N; i += kRed) z += raw[i];
    z = block_sum(z, red);
    double diff = 0.0, nd = 0.0, dg = 0.0;
    for (int i = threadIdx.x; i < N; i += kRed) {
        const double pn = raw[i] / z;
        diff += fabs(pn - p[i]);
        p[i] = pn;
        if (orp[i + 1] > orp[i])
            nd += pn;
        else
            dg += pn;
    }
    diff = block_sum(diff, red);
    nd = block_sum(nd, red);
    dg = block_sum(dg, red);
    if (threadIdx.x == 0) {
        const double it = scal[S_ITERS] + 1.0;
        scal[S_ND] = nd;
        scal[S_DG] = dg;
        scal[S_DIFF] = diff;
        scal[S_ITERS] = it;
        if (diff <= kFlowTol || it >= (double)max_iters) scal[S_DONE] = 1.0;
    }
}

__global__ void infomap_link_flow_kernel(const int* __restrict__ src, const double* __restrict__ w, const double* __restrict__ wout,
                                         const double* __restrict__ p, int E, double* __restrict__ q) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int i = src[e];
    q[e] = p[i] * w[e] / wout[i];
}

// one workgroup: *out = sum of v[0 .. n) (plogp of it with PLOGP) in a fixed order
template <bool PLOGP>
__global__ __launch_bounds__(kRed) void infomap_sum_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
    __shared__ double red[kRed];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kRed) s += PLOGP ? plogp(v[i]) : v[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) *out = s;
}

__global__ void infomap_scale_kernel(double* __restrict__ q, int E, const double* __restrict__ total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < E) q[e] = q[e] / *total;
}

// node flow = in-flow (in-links in ascending source order); iq = the link flows in in-list order
__global__ void infomap_node_flow_kernel(const int* __restrict__ irp, const int* __restrict__ ieid, const double* __restrict__ q, int N,
                                         double* __restrict__ iq, double* __restrict__ flow) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    double s = 0.0;
    for (int e = irp[j]; e < irp[j + 1]; ++e) {
        const double v = q[ieid[e]];
        iq[e] = v;
        s += v;
    }
    flow[j] = s;
}

// ---------------------------------------------------------------------------------------------- module totals, codelength
// xo[u] / xi[u] = flow of unit u's out / in links whose other end lies in another module
__global__ void infomap_cross_kernel(const int* __restrict__ orp, const int* __restrict__ odst, const double* __restrict__ oq,
                                     const int* __restrict__ irp, const int* __restrict__ isrc, const double* __restrict__ iq,
                                     const int* __restrict__ mod, int U, double* __restrict__ xo, double* __restrict__ xi) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const int a = mod[u];
    double so = 0.0, si = 0.0;
    for (int e = orp[u]; e < orp[u + 1]; ++e)
        if (mod[odst[e]] != a) so += oq[e];
    for (int e = irp[u]; e < irp[u + 1]; ++e)
        if (mod[isrc[e]] != a) si += iq[e];
    xo[u] = so;
    xi[u] = si;
}

// segment s = the units of one module in ascending unit index (order / segptr: a stable sort of mod); its sums go to slot mod
__global__ void infomap_module_totals_kernel(const int* __restrict__ order, const int* __restrict__ segptr, int S, int U,
                                             const int* __restrict__ mod, const double* __restrict__ xo, const double* __restrict__ xi,
                                             const double* __restrict__ pu, double* __restrict__ mexit, double* __restrict__ menter,
                                             double* __restrict__ mflow, int* __restrict__ nunits) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t0 = segptr[s], t1 = segptr[s + 1];
    if (t0 >= t1 || t0 < 0 || t1 > U) return;
    const int m = mod[order[t0]];
    if ((unsigned)m >= (unsigned)U) return;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int t = t0; t < t1; ++t) {
        const int u = order[t];
        a += xo[u];
        b += xi[u];
        c += pu[u];
    }
    mexit[m] = a;
    menter[m] = b;
    mflow[m] = c;
    nunits[m] = t1 - t0;
}

// one workgroup: out[0] = L of the module totals, out[1] = sum of enter flows
__global__ __launch_bounds__(kRed) void infomap_codelength_kernel(const double* __restrict__ mexit, const double* __restrict__ menter,
                                                                  const double* __restrict__ mflow, int M,
                                                                  const double* __restrict__ nodeterm, double* __restrict__ out) {
    __shared__ double red[kRed];
    double se = 0.0, pe = 0.0, px = 0.0, pf = 0.0;
    for (int m = threadIdx.x; m < M; m += kRed) {
        const double en = menter[m], ex = mexit[m];
        se += en;
        pe += plogp(en);
        px += plogp(ex);
        pf += plogp(ex + mflow[m]);
    }
    se = block_sum(se, red);
    pe = block_sum(pe, red);
    px = block_sum(px, red);
    pf = block_sum(pf, red);
    if (threadIdx.x == 0) {
        out[0] = plogp(se) - pe - px + pf - *nodeterm;
        out[1] = se;
    }
}

// ---------------------------------------------------------------------------------------------- search
// a positive gain's bits order like the gain; the low 16 bits carry the unit so that equal gains go to the lower unit
__device__ __forceinline__ unsigned long long move_key(double gain, int u) {
    return ((unsigned long long)__double_as_longlong(gain) & ~0xFFFFull) | (unsigned long long)(0xFFFF - u);
}

// One wavefront per unit u of module A.  Its list = out links then in links; entry f has the other unit's module c_f.  The
// lane that holds the first entry of a module B != A adds up u's flow to and from B over the whole list (front to back) and
// evaluates the move against the frozen module totals:
//   exit_A' = exit_A - exit_u + (out_uA + in_uA)      enter_A' = enter_A - enter_u + (out_uA + in_uA)
//   exit_B' = exit_B + exit_u - (out_uB + in_uB)      enter_B' = enter_B + enter_u - (out_uB + in_uB)
// (a module left empty gets exact zeros).  Any degree takes this one path: the work is degree^2, the state a few registers.
// Best gain above kMinGain, ties to the lower module: tgt / key / vals of the unit, and the key is raised on both modules
// and on *best (64-bit integer max: the winner does not depend on the order).
__global__ __launch_bounds__(256) void infomap_propose_kernel(const int* __restrict__ orp, const int* __restrict__ odst,
                                                              const double* __restrict__ oq, const int* __restrict__ irp,
                                                              const int* __restrict__ isrc, const double* __restrict__ iq,
                                                              const double* __restrict__ pu, const int* __restrict__ mod,
                                                              const double* __restrict__ mexit, const double* __restrict__ menter,
                                                              const double* __restrict__ mflow, const int* __restrict__ nunits, int U,
                                                              const double* __restrict__ cl, int* __restrict__ tgt,
                                                              unsigned long long* __restrict__ key, double* __restrict__ vals,
                                                              unsigned long long* claim, unsigned long long* best) {
    const int lane = threadIdx.x & 63, u = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (u >= U) return;
    const int o0 = orp[u], no = orp[u + 1] - o0, i0 = irp[u], ni = irp[u + 1] - i0, n = no + ni;
    const int A = mod[u];
    if (n == 0 || (unsigned)A >= (unsigned)U) {
        if (lane == 0) tgt[u] = -1;
        return;
    }
    auto entry_mod = [&](int f) { return mod[f < no ? odst[o0 + f] : isrc[i0 + f - no]]; };
    auto entry_q = [&](int f) { return f < no ? oq[o0 + f] : iq[i0 + f - no]; };
    double xu = 0.0, nu = 0.0, uA = 0.0;          // exit_u, enter_u, out_uA + in_uA
    for (int f = lane; f < n; f += 64) {
        const double q = entry_q(f);
        if (f < no)
            xu += q;
        else
            nu += q;
        if (entry_mod(f) == A) uA += q;
    }
    xu = wave_sum(xu);
    nu = wave_sum(nu);
    uA = wave_sum(uA);
    const bool last = nunits[A] == 1;
    const double eA = mexit[A], nA = menter[A], fA = mflow[A], p = pu[u], SE = cl[1];
    const double eA2 = last ? 0.0 : fmax(eA - xu + uA, 0.0), nA2 = last ? 0.0 : fmax(nA - nu + uA, 0.0);
    const double fA2 = last ? 0.0 : fmax(fA - p, 0.0);
    const double oldA = -plogp(nA) - plogp(eA) + plogp(eA + fA), newA = -plogp(nA2) - plogp(eA2) + plogp(eA2 + fA2);
    double bg = 0.0, bv2 = 0.0, bv3 = 0.0;
    int bB = INT_MAX;
    for (int f = lane; f < n; f += 64) {
        const int B = entry_mod(f);
        if (B == A || (unsigned)B >= (unsigned)U) continue;
        bool first = true;
        double uB = 0.0;
        for (int g = 0; g < n; ++g) {
            if (entry_mod(g) != B) continue;
            if (g < f) {
                first = false;
                break;
            }
            uB += entry_q(g);
        }
        if (!first) continue;
        const double eB = mexit[B], nB = menter[B], fB = mflow[B];
        const double eB2 = fmax(eB + xu - uB, 0.0), nB2 = fmax(nB + nu - uB, 0.0), fB2 = fB + p;
        const double SE2 = fmax(SE - nA - nB + nA2 + nB2, 0.0);
        const double dL = plogp(SE2) - plogp(SE) + newA - oldA - plogp(nB2) - plogp(eB2) + plogp(eB2 + fB2) + plogp(nB) + plogp(eB) -
                          plogp(eB + fB);
        const double gain = -dL;
        if (gain > kMinGain && (gain > bg || (gain == bg && B < bB))) {
            bg = gain;
            bB = B;
            bv2 = eB2;
            bv3 = nB2;
        }
    }
    double wg = bg;
    int wB = bB;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(wg, off, 64);
        const int ob = __shfl_xor(wB, off, 64);
        if (og > wg || (og == wg && ob < wB)) {
            wg = og;
            wB = ob;
        }
    }
    if (wB == INT_MAX) {
        if (lane == 0) tgt[u] = -1;
        return;
    }
    if (bB == wB) {                        // one lane: a module has one first entry
        const unsigned long long kk = move_key(wg, u);
        tgt[u] = wB;
        key[u] = kk;
        vals[4 * (int64_t)u + 0] = eA2;
        vals[4 * (int64_t)u + 1] = nA2;
        vals[4 * (int64_t)u + 2] = bv2;
        vals[4 * (int64_t)u + 3] = bv3;
        atomicMax(claim + A, kk);
        atomicMax(claim + wB, kk);
        atomicMax(best, kk);
    }
}

// single == 0: a unit moves if its key holds both its modules, so the admitted moves touch disjoint modules and each mover
// writes the totals of its two modules itself.  single == 1: only the unit that holds *best moves.
__global__ void infomap_apply_kernel(const int* __restrict__ tgt, const unsigned long long* __restrict__ key,
                                     const double* __restrict__ vals, const unsigned long long* __restrict__ claim,
                                     const unsigned long long* __restrict__ best, const double* __restrict__ pu, int U, int single,
                                     int* __restrict__ mod, double* __restrict__ mexit, double* __restrict__ menter,
                                     double* __restrict__ mflow, int* __restrict__ nunits, int* __restrict__ nmoved) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= U) return;
    const int B = tgt[u];
    if (B < 0) return;
    const int A = mod[u];
    const unsigned long long kk = key[u];
    if (single ? kk != *best : (claim[A] != kk || claim[B] != kk)) return;
    const bool last = nunits[A] == 1;
    mexit[A] = vals[4 * (int64_t)u + 0];
    menter[A] = vals[4 * (int64_t)u + 1];
    mexit[B] = vals[4 * (int64_t)u + 2];
    menter[B] = vals[4 * (int64_t)u + 3];
    mflow[A] = last ? 0.0 : fmax(mflow[A] - pu[u], 0.0);
    mflow[B] = mflow[B] + pu[u];
    nunits[A] -= 1;
    nunits[B] += 1;
    mod[u] = B;
    atomicAdd(nmoved, 1);
}

// ---------------------------------------------------------------------------------------------- aggregation
// out[s] = sum of q[eidx[t]] over segment s (the leaf links between one pair of modules, in ascending link index)
__global__ void infomap_segment_sum_kernel(const double* __restrict__ q, int E, const int* __restrict__ eidx,
                                           const int* __restrict__ segptr, int S, int T, double* __restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const int t0 = max(segptr[s], 0), t1 = min(segptr[s + 1], T);
    double a = 0.0;
    for (int t = t0; t < t1; ++t) {
        const int e = eidx[t];
        if ((unsigned)e < (unsigned)E) a += q[e];
    }
    out[s] = a;
}

// ---------------------------------------------------------------------------------------------- labels
__global__ void infomap_label_init_kernel(int N, int* __restrict__ size, int* __restrict__ minm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) {
        size[i] = 0;
        minm[i] = INT_MAX;
    }
}

__global__ void infomap_label_count_kernel(const int* __restrict__ mod, int N, int* size, int* minm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int m = mod[i];
    if ((unsigned)m >= (unsigned)N) return;
    atomicAdd(size + m, 1);
    atomicMin(minm + m, i);
}

// head[i] = i is the smallest member of a module with more than cluster_num members
__global__ void infomap_label_head_kernel(const int* __restrict__ mod, int N, int cluster_num, const int* __restrict__ size,
                                          const int* __restrict__ minm, int* __restrict__ head) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int m = mod[i];
    head[i] = (unsigned)m < (unsigned)N && minm[m] == i && size[m] > cluster_num;
}

// num = exclusive prefix sum of head: the kept modules numbered by ascending smallest member
__global__ void infomap_label_write_kernel(const int* __restrict__ mod, int N, int cluster_num, const int* __restrict__ size,
                                           const int* __restrict__ minm, const int* __restrict__ num, int64_t* __restrict__ labels) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int m = mod[i];
    const bool keep = (unsigned)m < (unsigned)N && size[m] > cluster_num;
    labels[i] = keep ? num[min(max(minm[m], 0), N - 1)] : -1;
}

inline bool table_ok(const int* nbrs, const float* dists, int N, int k) { return nbrs && dists && N > 0 && N <= kMaxN && k > 0 && k <= kMaxK; }
inline bool graph_ok(const int* orp, const int* irp, int N, int E) { return orp && irp && N > 0 && N <= kMaxN && E > 0; }

}  // namespace

extern "C" int rg_infomap_links_count(const int* nbrs, const float* dists, int N, int k, float thr, int* cnt, int* rowptr,
                                      hipStream_t stream) {
    RG_REQUIRE(table_ok(nbrs, dists, N, k) && cnt && rowptr, "rg_infomap_links_count: bad arguments (1 <= N <= %d, 1 <= k <= %d)", kMaxN,
               kMaxK);
    RG_REQUIRE(thr == thr, "rg_infomap_links_count: the threshold is NaN");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 8.0 * N * (double)k);
    hipLaunchKernelGGL((infomap_links_kernel<false>), dim3(rg::cdiv(N, kRowsPerBlock)), dim3(256), 0, stream, nbrs, dists, N, k, thr, cnt,
                       (const int*)nullptr, (int*)nullptr, (int*)nullptr, (double*)nullptr, (int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, cnt, N, rowptr);
    return rg::check_launch("rg_infomap_links_count");
}

extern "C" int rg_infomap_links_fill(const int* nbrs, const float* dists, int N, int k, float thr, const int* rowptr, int* src, int* dst,
                                     double* w, int* single, int* incnt, int* in_rowptr, hipStream_t stream) {
    RG_REQUIRE(table_ok(nbrs, dists, N, k) && rowptr && src && dst && w && single && incnt && in_rowptr,
               "rg_infomap_links_fill: bad arguments (1 <= N <= %d, 1 <= k <= %d)", kMaxN, kMaxK);
    RG_REQUIRE(thr == thr, "rg_infomap_links_fill: the threshold is NaN");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 8.0 * N * (double)k);
    if (hipMemsetAsync(incnt, 0, sizeof(int) * (size_t)N, stream) != hipSuccess) {
        rg::set_error("rg_infomap_links_fill: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL((infomap_links_kernel<true>), dim3(rg::cdiv(N, kRowsPerBlock)), dim3(256), 0, stream, nbrs, dists, N, k, thr,
                       (int*)nullptr, rowptr, src, dst, w, single, incnt);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, incnt, N, in_rowptr);
    return rg::check_launch("rg_infomap_links_fill");
}

extern "C" int rg_infomap_flow_start(const int* orp, const double* w, const int* irp, const int* ieid, int N, int E, double* wout,
                                     double* win, double* p, double* tele, double* scal, hipStream_t stream) {
    RG_REQUIRE(graph_ok(orp, irp, N, E) && w && ieid && wout && win && p && tele && scal,
               "rg_infomap_flow_start: bad arguments (1 <= N <= %d, at least one link)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(infomap_weights_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, orp, w, irp, ieid, N, wout, win);
    hipLaunchKernelGGL(infomap_flow_start_kernel, dim3(1), dim3(kRed), 0, stream, orp, irp, win, N, p, tele, scal);
    return rg::check_launch("rg_infomap_flow_start");
}

extern "C" int rg_infomap_flow_iterate(const int* orp, const int* irp, const int* isrc, const int* ieid, const double* w,
                                       const double* wout, const double* tele, int N, int E, int iters, int max_iters, double* p,
                                       double* raw, double* scal, hipStream_t stream) {
    RG_REQUIRE(graph_ok(orp, irp, N, E) && isrc && ieid && w && wout && tele && p && raw && scal,
               "rg_infomap_flow_iterate: bad arguments (1 <= N <= %d, at least one link)", kMaxN);
    RG_REQUIRE(iters >= 1 && iters <= 64 && max_iters >= 1, "rg_infomap_flow_iterate: need 1 <= iters <= 64 and max_iters >= 1, got %d, %d",
               iters, max_iters);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(infomap_flow_pull_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, irp, isrc, ieid, w, wout, p, tele, N, scal,
                           raw);
        hipLaunchKernelGGL(infomap_flow_update_kernel, dim3(1), dim3(kRed), 0, stream, orp, raw, N, p, scal, max_iters);
    }
    return rg::check_launch("rg_infomap_flow_iterate");
}

extern "C" int rg_infomap_flow_finish(const int* src, const int* irp, const int* ieid, const double* w, const double* wout,
                                      const double* p, int N, int E, double* q, double* iq, double* flow, double* scal,
                                      hipStream_t stream) {
    RG_REQUIRE(src && irp && ieid && w && wout && p && q && iq && flow && scal && N > 0 && N <= kMaxN && E > 0,
               "rg_infomap_flow_finish: bad arguments (1 <= N <= %d, at least one link)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(infomap_link_flow_kernel, dim3(rg::cdiv(E, 256)), dim3(256), 0, stream, src, w, wout, p, E, q);
    hipLaunchKernelGGL((infomap_sum_kernel<false>), dim3(1), dim3(kRed), 0, stream, (const double*)q, E, scal + S_Q);
    hipLaunchKernelGGL(infomap_scale_kernel, dim3(rg::cdiv(E, 256)), dim3(256), 0, stream, q, E, (const double*)(scal + S_Q));
    hipLaunchKernelGGL(infomap_node_flow_kernel, dim3(rg::cdiv(N, 256)), dim3(256), 0, stream, irp, ieid, (const double*)q, N, iq, flow);
    hipLaunchKernelGGL((infomap_sum_kernel<true>), dim3(1), dim3(kRed), 0, stream, (const double*)flow, N, scal + S_NODETERM);
    return rg::check_launch("rg_infomap_flow_finish");
}

extern "C" int rg_infomap_totals(const int* orp, const int* odst, const double* oq, const int* irp, const int* isrc, const double* iq,
                                 const double* pu, const int* mod, const int* order, const int* segptr, int U, int S, double* xo,
                                 double* xi, double* mexit, double* menter, double* mflow, int* nunits, hipStream_t stream) {
    RG_REQUIRE(orp && odst && oq && irp && isrc && iq && pu && mod && order && segptr && xo && xi && mexit && menter && mflow && nunits &&
                   U > 0 && U <= kMaxN && S > 0 && S <= U,
               "rg_infomap_totals: bad arguments (1 <= S <= U <= %d)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(infomap_cross_kernel, dim3(rg::cdiv(U, 256)), dim3(256), 0, stream, orp, odst, oq, irp, isrc, iq, mod, U, xo, xi);
    hipLaunchKernelGGL(infomap_module_totals_kernel, dim3(rg::cdiv(S, 256)), dim3(256), 0, stream, order, segptr, S, U, mod,
                       (const double*)xo, (const double*)xi, pu, mexit, menter, mflow, nunits);
    return rg::check_launch("rg_infomap_totals");
}

extern "C" int rg_infomap_codelength(const double* mexit, const double* menter, const double* mflow, int M, const double* nodeterm,
                                     double* out, hipStream_t stream) {
    RG_REQUIRE(mexit && menter && mflow && nodeterm && out && M > 0 && M <= kMaxN, "rg_infomap_codelength: bad arguments (1 <= M <= %d)",
               kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(infomap_codelength_kernel, dim3(1), dim3(kRed), 0, stream, mexit, menter, mflow, M, nodeterm, out);
    return rg::check_launch("rg_infomap_codelength");
}

extern "C" int rg_infomap_propose(const int* orp, const int* odst, const double* oq, const int* irp, const int* isrc, const double* iq,
                                  const double* pu, const int* mod, const double* mexit, const double* menter, const double* mflow,
                                  const int* nunits, int U, const double* cl, int* tgt, void* key, double* vals, void* claim, void* best,
                                  int* nmoved, hipStream_t stream) {
    RG_REQUIRE(orp && odst && oq && irp && isrc && iq && pu && mod && mexit && menter && mflow && nunits && cl && tgt && key && vals &&
                   claim && best && nmoved && U > 0 && U <= kMaxN,
               "rg_infomap_propose: bad arguments (1 <= U <= %d)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    if (hipMemsetAsync(claim, 0, sizeof(unsigned long long) * (size_t)U, stream) != hipSuccess ||
        hipMemsetAsync(best, 0, sizeof(unsigned long long), stream) != hipSuccess ||
        hipMemsetAsync(nmoved, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_infomap_propose: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(infomap_propose_kernel, dim3(rg::cdiv(U, kRowsPerBlock)), dim3(256), 0, stream, orp, odst, oq, irp, isrc, iq, pu,
                       mod, mexit, menter, mflow, nunits, U, cl, tgt, (unsigned long long*)key, vals, (unsigned long long*)claim,
                       (unsigned long long*)best);
    return rg::check_launch("rg_infomap_propose");
}

extern "C" int rg_infomap_apply(const int* tgt, const void* key, const double* vals, const void* claim, const void* best,
                                const double* pu, int U, int single, int* mod, double* mexit, double* menter, double* mflow, int* nunits,
                                int* nmoved, hipStream_t stream) {
    RG_REQUIRE(tgt && key && vals && claim && best && pu && mod && mexit && menter && mflow && nunits && nmoved && U > 0 && U <= kMaxN &&
                   (single == 0 || single == 1),
               "rg_infomap_apply: bad arguments (1 <= U <= %d, single 0 or 1)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    if (hipMemsetAsync(nmoved, 0, sizeof(int), stream) != hipSuccess) {
        rg::set_error("rg_infomap_apply: hipMemsetAsync failed");
        return RG_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(infomap_apply_kernel, dim3(rg::cdiv(U, 256)), dim3(256), 0, stream, tgt, (const unsigned long long*)key, vals,
                       (const unsigned long long*)claim, (const unsigned long long*)best, pu, U, single, mod, mexit, menter, mflow, nunits,
                       nmoved);
    return rg::check_launch("rg_infomap_apply");
}

extern "C" int rg_infomap_segment_sum(const double* q, int E, const int* eidx, const int* segptr, int S, int T, double* out,
                                      hipStream_t stream) {
    RG_REQUIRE(q && eidx && segptr && out && E > 0 && S > 0 && T > 0, "rg_infomap_segment_sum: bad arguments");
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    hipLaunchKernelGGL(infomap_segment_sum_kernel, dim3(rg::cdiv(S, 256)), dim3(256), 0, stream, q, E, eidx, segptr, S, T, out);
    return rg::check_launch("rg_infomap_segment_sum");
}

extern "C" int rg_infomap_labels(const int* mod, int N, int cluster_num, int* size, int* minm, int* head, int* num, int64_t* labels,
                                 hipStream_t stream) {
    RG_REQUIRE(mod && size && minm && head && num && labels && N > 0 && N <= kMaxN && cluster_num >= 0,
               "rg_infomap_labels: bad arguments (1 <= N <= %d, cluster_num >= 0)", kMaxN);
    rg::ProfScope prof(rg::FAM_MISC, stream, 0.0, 0.0);
    const dim3 grid(rg::cdiv(N, 256));
    hipLaunchKernelGGL(infomap_label_init_kernel, grid, dim3(256), 0, stream, N, size, minm);
    hipLaunchKernelGGL(infomap_label_count_kernel, grid, dim3(256), 0, stream, mod, N, size, minm);
    hipLaunchKernelGGL(infomap_label_head_kernel, grid, dim3(256), 0, stream, mod, N, cluster_num, (const int*)size, (const int*)minm, head);
    hipLaunchKernelGGL(rg_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream, (const int*)head, N, num);
    hipLaunchKernelGGL(infomap_label_write_kernel, grid, dim3(256), 0, stream, mod, N, cluster_num, (const int*)size, (const int*)minm,
                       (const int*)num, labels);
    return rg::check_launch("rg_infomap_labels");
}

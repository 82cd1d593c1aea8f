// rtx_query.h — batched ray queries of the resident scene (rtx_query,
// include/rtx_ray_query.h): for each caller ray the closest hit (Scene::intersect,
// scene.cpp:157-180) or the ordered list of all hits (Scene::intersectList +
// std::sort, light.cpp:25-26: the shadow walk's chain of next-hit queries).
//
// The per-ray logic — start a ray, act on a completed query (store the entry,
// translate the ids, restart from the answer or stop), fill the unused
// entries — is RT_HD, so the unit test (tests/native/query_host.hip) runs the
// same code on the host against the CPU restatement.  query_kernel (the
// device part, compiled where RTX_QUERY_KERNEL is defined: rtx_render.hip) is
// the persistent traversal of the un-fused trace_kernel around it.
#pragma once

#include "rtx_traverse.h"
#include "rtx_ray_query.h"

namespace rtxd {

// Where a batch's answers go: [n][kmax] entries (t, object, face: each may be
// null) and [n] counts (may be null).
struct QueryOut {
  double* t;
  int32_t* object;
  int32_t* face;
  int32_t* nhits;
  int32_t kmax;
};

// Ray k's first query; false if it is already complete (a miss: the root box).
template <int QMODE, class TR>
RT_HD bool query_begin(TR& T, const DevScene& S, const double* __restrict__ P, const double* __restrict__ D,
                       const size_t k, Counters& C) {
  const dvec3 p = mk3(P[3 * k], P[3 * k + 1], P[3 * k + 2]);
  const dvec3 d = mk3(D[3 * k], D[3 * k + 1], D[3 * k + 2]);
  return trav_init<false, QMODE>(T, S, p, d, -RTX_INF, -1, -1, RTX_INF, C);
}

// Entries [j, kmax) of ray k are unused, its list has j entries.
RT_HD void query_fill(const QueryOut& O, const size_t k, const int j) {
  for (int e = j; e < O.kmax; ++e) {
    const size_t at = k * static_cast<size_t>(O.kmax) + static_cast<size_t>(e);
    if (O.t) O.t[at] = 0.0;
    if (O.object) O.object[at] = -1;
    if (O.face) O.face[at] = -1;
  }
  if (O.nhits) O.nhits[k] = j;
}

// Ray k's query is complete (T.have, T.bt, T.bobj, T.bsub): a hit becomes
// entry j (the object's and the face's ids of the scene file), and an
// all-hits list with room left queries again from that hit's key — true: the
// lane goes on stepping.  False: the ray is done, all of its entries and its
// count are written.
template <int QMODE, class TR>
RT_HD bool query_complete(TR& T, const DevScene& S, const QueryOut& O, const size_t k, int& j, Counters& C) {
  while (T.have) {
    const double bt = T.bt;
    const int bo = T.bobj, bs = T.bsub;
    const size_t at = k * static_cast<size_t>(O.kmax) + static_cast<size_t>(j);
    const RtxObject& o = S.objs[bo];
    if (O.t) O.t[at] = bt;
    if (O.object) O.object[at] = o.orig_id;
    if (O.face) O.face[at] = o.type == RTX_OBJ_TRIMESH ? S.fids[S.meshes[o.mesh].face_off + bs].orig_id : -1;
    ++j;
    if (QMODE == Q_CLOSEST || j >= O.kmax) break;
    // (the ray from the walk's cold state: trav_init stores the same values back)
    const dvec3 p = T.cold.getP(), d = T.cold.getD();
    if (trav_init<false, QMODE>(T, S, p, d, bt, bo, bs, RTX_INF, C)) return true;
  }
  query_fill(O, k, j);
  return false;
}

}  // namespace rtxd

#ifdef RTX_QUERY_KERNEL
// waves per SIMD the kernel is bounded for: 3, as the trace kernels (at most
// 168 VGPRs).  The walk state alone takes about 150 (the un-fused
// trace_kernel's 149-151); bounded for 4 waves (128 VGPRs) every
// instantiation spills 76-108 bytes per lane (DESIGN.md "Ray queries")
#ifndef RTX_QUERY_WAVES
#define RTX_QUERY_WAVES 3
#endif

struct QueryArgs {
  const double* P;      // origins [n][3]
  const double* D;      // directions [n][3]
  QueryOut out;
  unsigned int n;       // rays (at most 2^31: the claims cannot wrap)
  unsigned int* claim;  // this batch's claim counter (0 at launch)
  int stack_cap;        // stack entries a walk can need
  int lds_k;            // SHORT: stack entries per lane in LDS
  int leaf_k;           // costly units wait while >= leaf_k lanes are at a record
  int* ovf;             // SHORT: overflow columns, [stack_cap - lds_k][threads of the launch]
};

// Persistent traversal of the caller's rays, in the mould of the un-fused
// trace_kernel: a wave claims 64 rays at a time (one atomic) and hands them to
// its idle lanes (ballot + mbcnt) once no lane is stepping any more (earlier
// refills measured slower there); costly units are postponed while enough
// lanes are at 4-wide records (while-while).  A lane whose query completes
// stores its entry at once and, in an all-hits list, restarts in place
// (query_complete).  LDS as trace_kernel's: per wave the stack — whole, or
// with SHORT its first lds_k entries, the rest in the overflow columns — then
// the cold state's [RTX_COLD_FIELDS][64] doubles.  No shading, no lane state
// in HBM, no counters but the claim: nothing of a render is touched.
template <int MODE, bool SHORT>
__global__ void __launch_bounds__(WG, RTX_QUERY_WAVES) query_kernel(DevScene S, QueryArgs A) {
  extern __shared__ int lds_stack[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int scap = SHORT ? A.lds_k : A.stack_cap;  // stack entries per lane in LDS
  using Stk = typename std::conditional<SHORT, StackShort, StackLDS>::type;
  Stk stk;
  if constexpr (SHORT)
    stk = StackShort{lds_stack + wave * scap * 64 + lane, lds_stack, A.ovf + blockIdx.x * WG,
                     static_cast<int>(gridDim.x) * WG, scap};
  else
    stk = StackLDS{lds_stack + wave * scap * 64 + lane};
  Counters C = {0, 0, 0, 0, 0, 0, 0};
  TravT<ColdLDS> T;
  T.cold.c = reinterpret_cast<double*>(lds_stack + WAVES_PER_WG * scap * 64) + wave * RTX_COLD_FIELDS * 64 + lane;
  const unsigned int nq = A.n;
  bool active = false;
  size_t k = 0;  // the lane's ray
  int j = 0;     // entries of its list so far
  // wave-uniform claim state: rays [qnext, qend)
  unsigned int qnext = 0, qend = 0;
  bool exhausted = false;
  for (;;) {
    unsigned long long idle = __ballot(!active);
    while (idle != 0ull && !exhausted) {
      if (qnext >= qend) {
        unsigned int base = nq;
        if (lane == 0) base = atomicAdd(A.claim, 64u);
        base = __shfl(base, 0);
        if (base >= nq) {
          exhausted = true;
          break;
        }
        qnext = base;
        qend = base + 64u < nq ? base + 64u : nq;
      }
      const unsigned int rank = lane_prefix(idle);
      const unsigned int avail = qend - qnext;
      const unsigned int nidle = __popcll(idle);
      const unsigned int take = avail < nidle ? avail : nidle;
      if (!active && rank < take) {
        k = RTX_CHK(CHK_QREC, static_cast<size_t>(qnext) + rank, nq);
        j = 0;
        active = query_begin<MODE>(T, S, A.P, A.D, k, C);
        if (!active) active = query_complete<MODE>(T, S, A.out, k, j, C);  // (a miss: the unused entries)
      }
      qnext += take;
      idle = __ballot(!active);
    }
    if (__ballot(active) == 0ull) break;  // nothing claimed and nothing left
    do {
      const unsigned long long at_rec = __ballot(active && trav_at_record(T));
      const bool go = active && (static_cast<int>(__popcll(at_rec)) < A.leaf_k || trav_at_record(T));
      if (go) {
        const bool qdone = trav_step<false, MODE>(T, S, stk, C);
        (void)RTX_CHK(CHK_STACK, T.sp, A.stack_cap + 1);
        if (qdone) active = query_complete<MODE>(T, S, A.out, k, j, C);
      }
    } while (__ballot(active) != 0ull);
  }
}
#endif  // RTX_QUERY_KERNEL

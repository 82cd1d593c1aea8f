// query_host.hip — TEST HARNESS: the per-ray logic of rtx_query
// (csrc/hip/rtx_query.h: query_begin / query_complete / query_fill, what
// query_kernel runs per lane) compiled for the HOST, so the unit test
// tests/test_query_host.py can compare it ray by ray with the CPU
// restatement's Scene::intersect / sorted intersectList without a GPU.  The
// loop below is query_kernel's for one lane: begin, step until the query
// completes, complete (store, restart or stop).  Built with
// --offload-host-only; never shipped, never used by the product.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../cs378hgraphics-raytracer_amd/csrc/hip/rtx_query.h"

using namespace rtxd;

namespace {
std::string g_err;

struct HostScene {
  DevScene S;
  TravTrees T;
  int stack_cap = 0;
};

bool make_scene(const RtxSceneDesc* d, HostScene& H) {
  std::memset(&H.S, 0, sizeof(H.S));
  DevScene& S = H.S;
  if (!build_trav_trees(d, H.T)) return false;
  S.sroot = H.T.sroot;
  S.snode4 = H.T.sn4.data();
  S.mnode4 = H.T.mn4.data();
  S.n_srec = static_cast<int32_t>(H.T.sn4.size());
  S.mroots = H.T.mroots.data();
  S.tfaces = H.T.tfaces.data();
  S.trank = H.T.trank.data();
  S.snodes = d->scene_nodes;
  S.objs = H.T.objs.data();  // with the mesh fields in pad (augment_objects)
  S.tmeta = H.T.tmeta.data();
  S.oprm = d->obj_params;
  S.mats = d->materials;
  S.meshes = d->meshes;
  S.mnodes = d->mesh_nodes;
  S.faces = d->faces;
  S.fids = d->face_ids;
  S.n_snodes = d->n_scene_nodes;
  S.n_objs = d->n_objects;
  S.margin = 1e-9 * scene_extent(d);
  S.lmargin = 1e-9 * mesh_extent(d);
  H.stack_cap = H.T.sneed + H.T.mneed + 2;
  return true;
}

template <int QMODE>
void run(const HostScene& H, int64_t n, const double* P, const double* D, const QueryOut& O) {
  std::vector<int> col(size_t(H.stack_cap + 4) * 64, 0);  // one lane's stack column
  const StackLDS stk{col.data()};
  Counters C = {0, 0, 0, 0, 0, 0, 0};
  for (int64_t r = 0; r < n; ++r) {
    const size_t k = static_cast<size_t>(r);
    Trav T;
    int j = 0;
    bool active = query_begin<QMODE>(T, H.S, P, D, k, C);
    if (!active) active = query_complete<QMODE>(T, H.S, O, k, j, C);
    while (active)
      if (trav_step<false, QMODE>(T, H.S, stk, C)) active = query_complete<QMODE>(T, H.S, O, k, j, C);
  }
}
}  // namespace

extern "C" {

const char* query_host_last_error(void) { return g_err.c_str(); }

// rtx_query's modes and outputs (include/rtx_ray_query.h) for host arrays; every output
// may be null.
int query_host_run(const RtxSceneDesc* d, int32_t mode, int64_t n, const double* P, const double* D, int32_t kmax,
                   double* t, int32_t* object, int32_t* face, int32_t* nhits) {
  if ((mode != RTX_QUERY_CLOSEST && mode != RTX_QUERY_ALL) || kmax < 1 || (mode == RTX_QUERY_CLOSEST && kmax != 1)) {
    g_err = "bad mode / kmax";
    return -1;
  }
  HostScene H;
  if (!make_scene(d, H)) {
    g_err = "malformed BVH";
    return -1;
  }
  const QueryOut O = {t, object, face, nhits, kmax};
  if (mode == RTX_QUERY_CLOSEST) run<Q_CLOSEST>(H, n, P, D, O);
  else run<Q_NEXT>(H, n, P, D, O);
  return 0;
}

}  // extern "C"

// rtw_refit.hip -- the refit of the triangle tree on the device (rtw_ctx_refit_triangles): the triangle records and every
// box recomputed from the caller's origin / u / v, the topology kept.  Two kernels, each one thread per node of one height of the schedule
// (rtw_refit.h): the leaf pass, then the inner nodes bottom-up, ONE LAUNCH PER HEIGHT -- the kernel boundary is the hand-off between a node
// and its children.  (A single launch that climbs with arrival counters hands boxes between workgroups of different XCDs through L2s that
// are not coherent with one another: not built.)
#include "rtw_refit.h"

namespace rtw {

#define RTW_REFIT_BLOCK 256u

// Height 0: thread t refits leaf node order[t] (at most 4 triangles) and counts the triangles tri_box refuses
__global__ __launch_bounds__(RTW_REFIT_BLOCK) void tri_refit_leaves_kernel(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv,
                                                                           const uint32_t *order, uint32_t count, uint32_t *bad) {
    const uint32_t t = blockIdx.x * RTW_REFIT_BLOCK + threadIdx.x;
    if (t >= count) return;
    const uint32_t refused = refit_leaf_node(nodes, leaf, list, ouv, order[t]);
    if (refused) atomicAdd(bad, refused);
}

// One height above: thread t joins the children's boxes of inner node order[t]; both were written by earlier launches
__global__ __launch_bounds__(RTW_REFIT_BLOCK) void tri_refit_inner_kernel(TriNode *nodes, const uint32_t *order, uint32_t count) {
    const uint32_t t = blockIdx.x * RTW_REFIT_BLOCK + threadIdx.x;
    if (t >= count) return;
    refit_inner_node(nodes, order[t]);
}

void launch_tri_refit(TriNode *nodes, DevTri *leaf, DevTri *list, const float *ouv, const uint32_t *order, const uint32_t *first,
                      uint32_t n_heights, uint32_t *bad, hipStream_t stream) {
    if (n_heights == 0) return;
    const uint32_t n_leaves = first[1] - first[0];
    hipLaunchKernelGGL(tri_refit_leaves_kernel, dim3((n_leaves + RTW_REFIT_BLOCK - 1) / RTW_REFIT_BLOCK), dim3(RTW_REFIT_BLOCK), 0, stream,
                       nodes, leaf, list, ouv, order + first[0], n_leaves, bad);
    for (uint32_t h = 1; h < n_heights; h++) {
        const uint32_t count = first[h + 1] - first[h];
        hipLaunchKernelGGL(tri_refit_inner_kernel, dim3((count + RTW_REFIT_BLOCK - 1) / RTW_REFIT_BLOCK), dim3(RTW_REFIT_BLOCK), 0, stream,
                           nodes, order + first[h], count);
    }
}

// The same climb for another tree of the format (the top-level tree over placements, rtw_mesh_move.hip)
void launch_refit_climb(TriNode *nodes, const uint32_t *order, const uint32_t *first, uint32_t n_heights, hipStream_t stream) {
    for (uint32_t h = 1; h < n_heights; h++) {
        const uint32_t count = first[h + 1] - first[h];
        hipLaunchKernelGGL(tri_refit_inner_kernel, dim3((count + RTW_REFIT_BLOCK - 1) / RTW_REFIT_BLOCK), dim3(RTW_REFIT_BLOCK), 0, stream,
                           nodes, order + first[h], count);
    }
}

} // namespace rtw

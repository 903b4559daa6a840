// rtw_mesh_move.hip -- the refit of the top-level tree over mesh placements on the device (rtw_ctx_move_mesh_instances): the
// placements take new poses, the mesh's root box may have moved (a triangle refit just before, on the same stream), the tree keeps its
// topology.  The placement pass is one thread per LEAF node of the top-level tree (mesh_top_refit_leaf, rtw_refit.h -- the definition the host
// form runs); the climb over the inner nodes has two forms, chosen by launch_mesh_move's caller:
//   per height   launch_refit_climb (rtw_refit.hip): the triangle refit's kernel, one launch per height -- the kernel boundary is the hand-off
//   one group    mesh_top_climb_kernel below: ONE launch of ONE workgroup that loops over the heights itself.  4.12 rejected a single-launch
//                climb because boxes would pass between workgroups on different XCDs; here every box is written and read by waves of one
//                workgroup, on one CU, through that CU's one vector L1.
#include "rtw_refit.h"

namespace rtw {

#define RTW_MESH_MOVE_BLOCK 256u
#define RTW_MESH_CLIMB_BLOCK 1024u

// Height 0: thread t refits leaf node order[t] -- the rows of its at most 4 placements from `poses` (null: they stay), their world boxes from
// the mesh tree's node 0 as the device holds it now -- and counts the invalid poses and the placements beyond reach
__global__ __launch_bounds__(RTW_MESH_MOVE_BLOCK) void mesh_top_refit_leaves_kernel(TriNode *top, const uint32_t *top_order, f4 *rows, const float *poses,
                                                                                    const TriNode *root, const uint32_t *order, uint32_t count,
                                                                                    uint32_t *counts) {
    const uint32_t t = blockIdx.x * RTW_MESH_MOVE_BLOCK + threadIdx.x;
    if (t >= count) return;
    const TriNode r = *root;
    const MeshMoveCount n = mesh_top_refit_leaf(top, top_order, rows, poses, r, order[t]);
    if (n.invalid) atomicAdd(counts, n.invalid);
    if (n.beyond) atomicAdd(counts + 1, n.beyond);
}

// Heights 1 .. n_heights - 1 in one launch of ONE workgroup: the threads stride over order[first[h] .. first[h + 1]), then meet.
// The hand-off between a node and its children: a child's box is a plain global store of one wave, the parent's read a plain global load of
// another wave OF THIS WORKGROUP one height later.  __syncthreads() ALONE DOES NOT ORDER THEM: its fences cover LDS only, and with no LDS
// traffic it compiles to a bare s_barrier that waits for no counter -- a wave would arrive with its stores still in flight.  What orders them,
// in this order:
//   1. every wave waits for its own stores to be complete: `s_waitcnt vmcnt(0)`, written out (the compiler may drop the wait a fence implies
//      when it believes the counter empty), and a workgroup-scope RELEASE fence over all address spaces, so that no store is moved below it;
//   2. the barrier;
//   3. a workgroup-scope ACQUIRE fence, so that no load of the next height is moved above the barrier or served from a register.
// Workgroup scope suffices because all waves of a workgroup run on one CU and reach memory through that CU's one vector L1, which a store
// writes through: a completed store of one wave is what any wave of the same workgroup loads.  It would NOT suffice between workgroups
// (another CU's L1 may hold the old line, another XCD's L2 too): that is the reason the grid is 1, and why no other workgroup reads these
// nodes before the kernel has ended.
__global__ __launch_bounds__(RTW_MESH_CLIMB_BLOCK) void mesh_top_climb_kernel(TriNode *nodes, const uint32_t *order, const uint32_t *first,
                                                                              uint32_t n_heights) {
    for (uint32_t h = 1; h < n_heights; h++) {
        const uint32_t end = first[h + 1];
        for (uint32_t i = first[h] + threadIdx.x; i < end; i += RTW_MESH_CLIMB_BLOCK) refit_inner_node(nodes, order[i]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
}

// rtw_ctx_mesh_instance_motion: thread t forms the motion row of placement t (mesh_motion_row, rtw_refit.h -- the definition the host form runs)
// in registers and stores its 128 bytes as eight 16-byte stores: the rows of consecutive threads are consecutive in memory, so a wave's
// stores of one slot cover 64 lines that the next seven slots complete in L2.
__global__ __launch_bounds__(RTW_MESH_MOVE_BLOCK) void mesh_motion_kernel(const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows,
                                                                          uint32_t *n_invalid) {
    const uint32_t t = blockIdx.x * RTW_MESH_MOVE_BLOCK + threadIdx.x;
    if (t >= n) return;
    float prev[7], cur[7];
    for (int k = 0; k < 7; k++) { prev[k] = prev_poses[7 * (size_t)t + k]; cur[k] = cur_poses[7 * (size_t)t + k]; }
    RtwMotionRow r;
    const bool invalid = mesh_motion_row(prev, cur, r);
    rows[t] = r;
    if (invalid) atomicAdd(n_invalid, 1u);
}

void launch_mesh_motion(const float *prev_poses, const float *cur_poses, uint32_t n, RtwMotionRow *rows, uint32_t *n_invalid, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_motion_kernel, dim3((n + RTW_MESH_MOVE_BLOCK - 1) / RTW_MESH_MOVE_BLOCK), dim3(RTW_MESH_MOVE_BLOCK), 0, stream, prev_poses,
                       cur_poses, n, rows, n_invalid);
}

// rtw_ctx_deform_motion: thread p runs deform_point (rtw_refit.h -- the definition the host form runs) for pixel p.  The nine floats of a
// previous triangle are a gather (neighbouring pixels mostly share a triangle); tri, bary and the two results are consecutive per lane.
__global__ __launch_bounds__(RTW_MESH_MOVE_BLOCK) void deform_motion_kernel(const int32_t *tri, const float *bary, uint32_t n, DeformMesh m, float *point,
                                                                            float *normal) {
    const uint32_t p = blockIdx.x * RTW_MESH_MOVE_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float2 ab = *reinterpret_cast<const float2 *>(bary + 2 * (size_t)p);
    float x[3], nr[3];
    deform_point(m, tri[p], ab.x, ab.y, m.prev_poses ? m.idx[p] : 0, x, nr);
    *reinterpret_cast<float3 *>(point + 3 * (size_t)p) = make_float3(x[0], x[1], x[2]);
    *reinterpret_cast<float3 *>(normal + 3 * (size_t)p) = make_float3(nr[0], nr[1], nr[2]);
}

void launch_deform_motion(const int32_t *tri, const float *bary, uint32_t n, const DeformMesh &m, float *point, float *normal, hipStream_t stream) {
    hipLaunchKernelGGL(deform_motion_kernel, dim3((n + RTW_MESH_MOVE_BLOCK - 1) / RTW_MESH_MOVE_BLOCK), dim3(RTW_MESH_MOVE_BLOCK), 0, stream, tri, bary, n,
                       m, point, normal);
}

void launch_mesh_move(TriNode *top, const uint32_t *top_order, f4 *rows, const float *poses, const TriNode *root, const uint32_t *order,
                      const uint32_t *first, const uint32_t *d_first, uint32_t n_heights, bool one_group, uint32_t *counts, hipStream_t stream) {
    if (n_heights == 0) return;
    const uint32_t n_leaves = first[1] - first[0];
    hipLaunchKernelGGL(mesh_top_refit_leaves_kernel, dim3((n_leaves + RTW_MESH_MOVE_BLOCK - 1) / RTW_MESH_MOVE_BLOCK), dim3(RTW_MESH_MOVE_BLOCK), 0,
                       stream, top, top_order, rows, poses, root, order + first[0], n_leaves, counts);
    if (n_heights < 2) return;
    if (one_group) hipLaunchKernelGGL(mesh_top_climb_kernel, dim3(1), dim3(RTW_MESH_CLIMB_BLOCK), 0, stream, top, order, d_first, n_heights);
    else launch_refit_climb(top, order, first, n_heights, stream);
}

} // namespace rtw

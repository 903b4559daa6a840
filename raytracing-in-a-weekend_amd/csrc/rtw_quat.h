// rtw_quat.h -- Rust2's quaternion rotation of an `Instance` (Rust2/src/quaternions.rs:113-191, objects/instance.rs:215-255).  The pure
// pieces are __host__ __device__, one definition for the quaternion build of the render kernels (SPEC 11), for the query kernel
// (rtw_query.hip) and for the host entry points rtw_quat_rotate / rtw_quat_mul / rtw_quat_from_axis / rtw_quat_from_euler (rtw_shim.hip) that
// the CPU tests call.  f32, one rounding per written operation, no FMA (-ffp-contract=off), the reference's operation order.
//
// `Quaternion::rotate(v)` = qn.hamilton((0, v)).hamilton(qn.conjugate()).get_vec() with qn = q * (1.0 / q.len()).  qn depends on the instance
// alone: the host forms it once (quat_normalised) and uploads one f4 row {w, x, y, z} per instance; the conjugate is three exact negations.
// Every product with the literal w = 0 of From<&Vec3> is KEPT: it is +-0 (qn is finite), and dropping it would flip the sign of a zero sum
// (0 - x * 0 is +0 where -(x * 0) is -0).  The w component of the second product is never read and is not formed.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rtw {

struct quat { float w, x, y, z; };
__host__ __device__ __forceinline__ quat qmk(float w, float x, float y, float z) { quat q; q.w = w; q.x = x; q.y = y; q.z = z; return q; }

// Quaternion::hamilton (quaternions.rs:141-149): four products per component, added left to right
__host__ __device__ __forceinline__ quat quat_hamilton(quat a, quat b) {
    return qmk(a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
               a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
               a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x,
               a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w);
}
// Quaternion::len (:135-137)
__host__ __device__ __forceinline__ float quat_len(quat q) { return __builtin_sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z); }
// `self * (1.0 / self.len())` (:181): the quaternion the rotation is carried out with
__host__ __device__ __forceinline__ quat quat_normalised(quat q) {
    const float s = 1.0f / quat_len(q);
    return qmk(q.w * s, q.x * s, q.y * s, q.z * s);
}
// The rest of Quaternion::rotate (:182-185) for a qn that is already normalised: out = (qn (0, v) conj(qn)).get_vec()
__host__ __device__ __forceinline__ void quat_rotate_n(quat qn, float vx, float vy, float vz, float &ox, float &oy, float &oz) {
    const quat h = quat_hamilton(qn, qmk(0.0f, vx, vy, vz));
    const float cw = qn.w, cx = -qn.x, cy = -qn.y, cz = -qn.z;          // conjugate (:150-157)
    ox = h.w * cx + h.x * cw + h.y * cz - h.z * cy;
    oy = h.w * cy - h.x * cz + h.y * cw + h.z * cx;
    oz = h.w * cz + h.x * cy - h.y * cx + h.z * cw;
}
// Quaternion::rotate (:180-186)
__host__ __device__ __forceinline__ void quat_rotate(quat q, float vx, float vy, float vz, float &ox, float &oy, float &oz) {
    quat_rotate_n(quat_normalised(q), vx, vy, vz, ox, oy, oz);
}

// (host only)
// Quaternion::new_from_axis (:114-123): the axis through Vec3::unit (self / self.length()), sin / cos of angle * 0.5 from the platform libm
inline quat quat_from_axis(float angle, float ax, float ay, float az) {
    const float l = __builtin_sqrtf(ax * ax + ay * ay + az * az);
    const float ux = ax / l, uy = ay / l, uz = az / l;
    const float half = angle * 0.5f;
    const float s = sinf(half);
    return qmk(cosf(half), s * ux, s * uy, s * uz);
}
// From<&EulerAngles> (:68-85)
inline quat quat_from_euler(float ex, float ey, float ez) {
    const float cx = cosf(ex), cy = cosf(ey), cz = cosf(ez);
    const float sx = sinf(ex), sy = sinf(ey), sz = sinf(ez);
    return qmk(cx * cy * cz + sx * sy * sz, sx * cy * cz - cx * sy * sz, cx * sy * cz - sx * cy * sz, cx * cy * sz - sx * sy * cz);
}

} // namespace rtw

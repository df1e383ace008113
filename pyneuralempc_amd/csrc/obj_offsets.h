// Layout of the objective table (Handle::d_obj, and the table over an augmented stage: stage_aug.h).  Nothing of HIP and
// nothing of the library, so that host programs lay a table out the way the kernels read it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_OBJ_HD __host__ __device__
#else
#define NEMPC_OBJ_HD
#endif

namespace nempc {

struct ObjOffsets {  // element offsets into Handle::d_obj
    int Q, Qs, R, Rs, xref, uref, cx, cu, QT, QTs, total;   // QT: weight of the last step (terminal cost), QTs = QT + QT^T
};
NEMPC_OBJ_HD inline ObjOffsets obj_offsets(int H, int nx, int nu) {
    ObjOffsets o;
    int p = 0;
    o.Q = p; p += nx * nx;
    o.Qs = p; p += nx * nx;
    o.R = p; p += nu * nu;
    o.Rs = p; p += nu * nu;
    o.xref = p; p += H * nx;
    o.uref = p; p += H * nu;
    o.cx = p; p += H * nx;
    o.cu = p; p += H * nu;
    o.QT = p; p += nx * nx;
    o.QTs = p; p += nx * nx;
    o.total = p;
    return o;
}

}  // namespace nempc

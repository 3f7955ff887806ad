// object_types.hpp -- the plain records of the object update that the host fills (host/object_stage.hpp) and the kernels read
// (object_kernels.hpp, object_rows.hpp, object_fused.hpp).  Plain C++ (no HIP): declared once, here.
#pragma once

namespace orcvio_amd {

// one (object, clone) group of rows: [r0, r1) into ridx, which lists the rows of the update grouped by (object, clone)
struct ObjGroup { int r0, r1, clone, obj; };
// rows [row0, row0 + rows) of the update; K keypoint blocks; kp_off: first of the object's K + 1 (begin, end) pairs in the keypoint
// ranges, which index kp_rows: the rows of keypoint block 0 .. K-1, then the border-only rows
struct ObjArrow { int row0, rows, K, kp_off; };
// one object track of a row-evaluation launch (k_object_rows_batch, k_obj_fused)
struct ObjEvalArgs {
    const double* wTo;        // [16]
    const double* shape;      // [3]
    const double* kps;        // [K][3]
    const double* frame_wTc;  // [F][16]
    const double* frame_zs;   // [F][K][2]
    const double* frame_bbox; // [F][4]
    const int* frame_clone;   // [F] (-1: not in the window)
    const int* frame_row0;    // [F] first output row of the frame (only for in-window frames)
    int K, F, ncol;           // ncol = 9 + 3K
    int ldhf;                 // leading dimension of Hf (>= ncol; the columns beyond ncol are written as 0)
    int rcol;                 // >= ncol: the residual is ALSO written to column rcol of the Hf row (compact [Hf | r] rows of the
                              // object compression, msckf_kernels.hpp k_obj_cross); -1: not
    int* row_cols;            // optional: ncol of the object is written per row
    int obj_left, new_bbox, vio_left, fix_D;
    double R_b2c[9], t_c_b[3];
    int* row_clone;
    double* Hx6;
    double* Hf;
    double* res;
};

}  // namespace orcvio_amd

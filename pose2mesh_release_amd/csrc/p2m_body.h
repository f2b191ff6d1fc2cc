// Tile sizes, caps and the per-sample forward workspace layout of the body-model layer, shared by the forward (body.hip)
// and the backward (body_bwd.hip).
#pragma once
#include "p2m_common.h"

namespace p2m {

constexpr int BODY_VT = 64;                 // vertices per block of k_body_skin / k_body_bwd_vertex
constexpr int BODY_NT = BODY_VT * 3;        // threads: one per vertex component
constexpr int BODY_TB = 8;                  // samples per block
constexpr int BODY_JMAX = 64;               // chain joints / joints of the extra regressor
constexpr int BODY_KMAX = 640;              // coefficients: nb + 9 (J - 1) (SMPL 217, MANO 145)

// floats per sample of the forward workspace: [coef, K padded to 4 | A, 12 J | offset, 4]
__host__ __device__ inline int body_ws_floats(int J, int K) { return ((K + 3) / 4) * 4 + 12 * J + 4; }

}  // namespace p2m

// Where the forward-mode kernels that keep a point's rows in ONE lane put them (k_sdf_hessian, sdf_hess.hip; k_deform_kinematics,
// deform_kin.hip).  The MFMA result has col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5): a lane half owns 16 rows of
// each 32-row tile, as four quads.  Those rows, across the tile's row tiles, are the half's SLOTS (slot = 16 ri + reg: 32 on the 64-row
// tile, 16 on the 32-row tile), and a point takes consecutive slots of one half, so every product of its rows is between registers of
// one lane and a quad is still four consecutive rows.
#pragma once

namespace es {

// the tile row of slot s of lane half hi
__host__ __device__ constexpr int hess_row(int s, int hi) { return 32 * (s >> 4) + 8 * ((s >> 2) & 3) + 4 * hi + (s & 3); }
// and back: the slot of tile row r (its lane half is (r >> 2) & 1)
__host__ __device__ constexpr int hess_slot(int r) { return 16 * (r >> 5) + 4 * ((r >> 3) & 3) + (r & 3); }

}  // namespace es

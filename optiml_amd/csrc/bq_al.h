// Augmented-Lagrangian driver: internal declarations (the state structs live in bq_common.h next to bq_solver).
#pragma once
#include "bq_common.h"

constexpr int BQ_AL = 4;   // internal solver kind (created by bq_al_solver_create)

// the closing kernels' view of an AL solver (bq_epilogue.h, kind 2): sgn and q are the problem's; the batched solver
// (bq_msolver.hip) replaces sgn by its column's labels
bq_epilogue bq_al_epilogue(bq_solver *s);

// adapter_ragged.h -- internal (not part of the C ABI): the per-image layout of slime_adapter_forward_ragged, passed to the plan
// kernel BY VALUE in its kernel arguments (no upload, no host memory read after the call returns, capturable) -- hence the cap of
// SLIME_ADAPTER_RAGGED_MAX_IMAGES images: 1.3 KB of arguments.
#pragma once
#include "slime_hip.h"

struct RaggedLayout {
    int n_images, P, q, g, merge;                            // q = g*g rows per local crop (1 when no image has local crops)
    int crop0[SLIME_ADAPTER_RAGGED_MAX_IMAGES];              // index of image i's global crop in feats; its local crops follow it
    int n[SLIME_ADAPTER_RAGGED_MAX_IMAGES];                  // local crops of image i
    int nw[SLIME_ADAPTER_RAGGED_MAX_IMAGES];                 // columns of its crop grid (>= 1)
    int dst0[SLIME_ADAPTER_RAGGED_MAX_IMAGES];               // its first row in the token buffer
    int lrow0[SLIME_ADAPTER_RAGGED_MAX_IMAGES + 1];          // prefix of its local GEMM rows: image i owns local rows [lrow0[i], lrow0[i+1])
};

// rowwise.hip
int adapter_ragged_plan_launch(const RaggedLayout& L, int* row_map, int* glob_crops, int* local_crops, void* stream);
int select_crops_indexed_launch(const void* feats, int dtype, int P, int C, const int* table, int n_crops, float* out_f32, void* out_t,
                                void* stream);
int layernorm_crops_indexed_launch(const void* feats, int dtype, int P, const int* table, int n_crops, int D, const float* w, const float* b,
                                   float eps, void* out_t, void* out_t2, const float* add, int add_period, void* stream);

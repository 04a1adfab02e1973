// Spectral normalisation (spectral.hip): the plan and the launches behind vg_spectral_* of include/vitgan_hip.h.
#pragma once
#include "../../include/vitgan_hip.h"
#include "vg_common.h"

// fills the planned fields of tab[0..n) from (w_off, N, K); blocks (nullable) receives the three grid sizes.  -2: N or K < 1
int vg_spectral_plan_host(VgSpectralDesc* tab, int n, long long* state_floats, long long* scratch_floats, int* blocks);
int vg_spectral_update_launch(const float* W, bf16* shadow, float* state, float* scratch, const VgSpectralDesc* tab_dev, int n, const int* blocks,
                              int iterate, hipStream_t st);
int vg_spectral_project_launch(float* G, const float* W, const float* state, float* scratch, const VgSpectralDesc* tab_dev, int n, const int* blocks,
                               hipStream_t st);

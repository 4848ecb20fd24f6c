// The nine-tap 3x3 weight gradient (conv_wgrad3.hip) as the weight-gradient dispatch (conv_wgrad.hip: plan_wgrad) sees it.
#pragma once
#include "common.h"

// ok: the kernel serves the layer (3x3, stride 1, pad == dilation, bf16, Cout % 128 == 0, Cin % 64 == 0, >= 8192 pixels; hook sl_debug_wgrad3(0): never);
// the rest is the launch: polyphase geometry, pieces per strip / per block, splits, output tiles and the slab bytes
struct Wg3Plan { int ok, d, Hs, Ws, nstrips, L, SP, ppu, pieces, ppb, splits, tilesN, tilesC; size_t ws_bytes; };

Wg3Plan wg3_plan(const SlConvDesc* d);      // a cost-model search (up to 5 x 1024 candidates): once per call
// runs a plan with ok != 0; the caller has checked the workspace against pl.ws_bytes
int sl_wgrad3_run(const SlConvDesc* d, const Wg3Plan& pl, const void* x, const void* x2, const void* dy, float* dw, int dw_cin_total, int dw_ci_off, void* workspace, hipStream_t st);

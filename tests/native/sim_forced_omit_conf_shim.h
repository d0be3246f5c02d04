// tests/native/sim_forced_omit_conf_shim.h -- TEST ONLY: what csrc/ta_forced_omit_conf.hip uses beyond
// tests/native/hipshim and sim_forced_shim.h.  Its forward fill is the aligner's with omission (the prefix max-scan of
// sim_forced_omit_shim.h's controls), its backward fill takes values from the lane on the RIGHT and runs a SUFFIX max-scan.
// This header states what the hardware does for every control the kernel uses (CDNA3 / CDNA4 ISA, "Data Parallel
// Primitives"), built on sim_exchange, and the kernel's calls are routed here.  bound_ctrl is off everywhere: a lane
// without a source keeps `old`.
//   0x101 .. 0x10f  row_shl:n    lane p of a row of 16 takes lane p + n of ITS row, none for p + n > 15      (new here)
//   0x111 .. 0x11f  row_shr:n    lane p of a row of 16 takes lane p - n of ITS row, none for p < n
//   0x130           wave_shl:1   lane l takes lane l + 1, none for lane 63
//   0x138           wave_shr:1   lane l takes lane l - 1, none for lane 0
//   0x142           row_bcast:15 every lane of rows 1 .. 3 takes lane 15 of the row before, none in row 0
//   0x143           row_bcast:31 every lane of rows 2 and 3 takes lane 31, none in rows 0 and 1
// row_mask bit r enables the write in row r; bank_mask must be 0xf.
//   v_readlane_b32 (__builtin_amdgcn_readlane)  every lane gets lane `from`'s value, 0 <= from <= 63, the same `from` in
//                                               every lane                                                     (new here)
#pragma once
#include "sim_forced_shim.h"

inline int sim_omit_conf_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    if (bank_mask != 0xf || bound_ctrl) __builtin_trap();
    const int lane = (int)threadIdx.x, row = lane / 16, p = lane % 16;
    int from = -1;
    if (ctrl >= 0x101 && ctrl <= 0x10f) from = p + (ctrl - 0x100) <= 15 ? lane + (ctrl - 0x100) : -1;
    else if (ctrl >= 0x111 && ctrl <= 0x11f) from = p >= ctrl - 0x110 ? lane - (ctrl - 0x110) : -1;
    else if (ctrl == 0x130) from = lane < 63 ? lane + 1 : -1;
    else if (ctrl == 0x138) from = lane - 1;
    else if (ctrl == 0x142) from = row >= 1 ? 16 * row - 1 : -1;
    else if (ctrl == 0x143) from = row >= 2 ? 31 : -1;
    else __builtin_trap();
    if (!((row_mask >> row) & 1)) from = -1;
    return (int)sim_exchange((unsigned)src, [=](const unsigned long long* s) {
        return from >= 0 ? s[from] : (unsigned long long)(unsigned)old;
    });
}
#define __builtin_amdgcn_update_dpp sim_omit_conf_update_dpp

inline int sim_omit_conf_readlane(int v, int from) {
    if (from < 0 || from > 63) __builtin_trap();
    return (int)sim_exchange((unsigned)v, [=](const unsigned long long* s) { return s[from]; });
}
#define __builtin_amdgcn_readlane sim_omit_conf_readlane

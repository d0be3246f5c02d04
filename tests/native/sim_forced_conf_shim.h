// tests/native/sim_forced_conf_shim.h -- TEST ONLY: what csrc/ta_forced_conf.hip uses beyond tests/native/hipshim and
// sim_forced_shim.h.  Its backward fill takes values from the lane on the RIGHT, a DPP control the shim does not know;
// this header states what the hardware does for the two controls the kernel uses (CDNA3 / CDNA4 ISA, "Data Parallel
// Primitives"), built on sim_exchange, and the kernel's calls are routed here.  bound_ctrl is off: a lane without a source
// keeps `old`.
//   0x130  wave_shl:1   lane l takes lane l + 1, none for lane 63
//   0x138  wave_shr:1   lane l takes lane l - 1, none for lane 0
// row_mask and bank_mask must be 0xf.
#pragma once
#include "sim_forced_shim.h"

inline int sim_conf_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    if (row_mask != 0xf || bank_mask != 0xf || bound_ctrl) __builtin_trap();
    const int lane = (int)threadIdx.x;
    int from = -1;
    if (ctrl == 0x130) from = lane < 63 ? lane + 1 : -1;
    else if (ctrl == 0x138) from = lane - 1;
    else __builtin_trap();
    return (int)sim_exchange((unsigned)src, [=](const unsigned long long* s) {
        return from >= 0 ? s[from] : (unsigned long long)(unsigned)old;
    });
}
#define __builtin_amdgcn_update_dpp sim_conf_update_dpp

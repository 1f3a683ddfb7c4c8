// libextrack_hip.so: gap-aware register-resident 2-state likelihood kernels (xt_reg2.h, GAPS), frame_len 4.  See xt_reg2_gaps_inst.h.
#define XT_R2_F 4
#include "xt_reg2_gaps_inst.h"

// libextrack_hip.so: gap-aware register-resident 2-state gradient kernels (xt_reg2.h, NP > 0, GAPS), frame_len 6.  See xt_reg2_grad_gaps_inst.h.
#define XT_R2_F 6
#include "xt_reg2_grad_gaps_inst.h"

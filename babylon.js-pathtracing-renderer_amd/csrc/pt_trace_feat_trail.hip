// pt_trace_feat_trail.hip — the megakernel variants of the trail walk that stage the G-buffer for the feature buffers.
#define PT_WALK_NAME trail
#define PT_WALK_PROGS PT_FOR_EACH_PROG_TRAIL
#include "pt_trace_feat_inst.h"

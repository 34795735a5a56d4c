// pt_trace_feat_pairs.hip — the megakernel variants of the pairs walk that stage the G-buffer for the feature buffers.
#define PT_WALK_NAME pairs
#define PT_WALK_PROGS PT_FOR_EACH_PROG_PAIRS
#include "pt_trace_feat_inst.h"

// pt_trace_feat_ref.hip — the megakernel variants of the ref walk that stage the G-buffer for the feature buffers.
#define PT_WALK_NAME ref
#define PT_WALK_PROGS PT_FOR_EACH_PROG_REF
#include "pt_trace_feat_inst.h"

// The clean stage of a call that exports the graphs (ma_assemble_graph_batch): clean.hip once more, with the marks and the
// write-back of the LDS images compiled in -- k_clean_gx, k_clean_tail_gx and run_clean_pass_gx.  Kept in a translation unit of
// its own so that the kernels of every other call are compiled from exactly the code they were compiled from before
// (clean.hip, at MA_CLEAN_GX).
#define MA_CLEAN_GX 1
#include "clean.hip"

// k_debug_fe_pair.hip -- k_debug_fe.hip once more, for the object the Makefile builds with the range kernel's flags (BITSFLAGS)
#define ACT_DEBUG_FE_PAIR 1
#include "k_debug_fe.hip"

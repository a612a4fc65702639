// part 0 of the AIR check kernels (split only to parallelise compilation)
#define CM_CHECK_PART 0
#include "kernels_check.inc"

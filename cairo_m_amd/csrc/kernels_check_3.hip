// part 3 of the AIR check kernels (split only to parallelise compilation)
#define CM_CHECK_PART 3
#include "kernels_check.inc"

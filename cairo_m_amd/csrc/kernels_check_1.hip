// part 1 of the AIR check kernels (split only to parallelise compilation)
#define CM_CHECK_PART 1
#include "kernels_check.inc"

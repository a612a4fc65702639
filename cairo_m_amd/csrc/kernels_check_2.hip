// part 2 of the AIR check kernels (split only to parallelise compilation)
#define CM_CHECK_PART 2
#include "kernels_check.inc"

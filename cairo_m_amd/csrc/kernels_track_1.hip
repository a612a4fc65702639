// part 1 of the relation tracker kernels (split only to parallelise compilation)
#define CM_TRACK_PART 1
#include "kernels_track.inc"

// part 0 of the relation tracker kernels (split only to parallelise compilation)
#define CM_TRACK_PART 0
#include "kernels_track.inc"

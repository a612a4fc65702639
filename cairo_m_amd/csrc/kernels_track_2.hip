// part 2 of the relation tracker kernels (split only to parallelise compilation)
#define CM_TRACK_PART 2
#include "kernels_track.inc"

// k_verify_oods for component group 1 (verify_prelude_oods.inc; the groups: verify_prelude.hpp verify_oods_group)
#define CM_OODS_GROUP 1
#include "verify_prelude_oods.inc"

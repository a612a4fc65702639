// k_verify_oods for component group 3 (verify_prelude_oods.inc; the groups: verify_prelude.hpp verify_oods_group)
#define CM_OODS_GROUP 3
#include "verify_prelude_oods.inc"

// The BDPT megakernel for scenes whose BSDF records do not fit the LDS table
// budget (more than ~300 materials): the same source as bdpt_kernels.hip with
// the records read from HBM (BDPT_BSDF_TABLE 1, bsdf_of in dev_scene.hpp);
// every host-visible symbol gets an _hbm name. Selected by bdpt_ctx_create's
// table layout (DevScene::lds_bsdf_off == kNoLds).
#define BDPT_BSDF_TABLE 1
#define BDPT_VARIANT _hbm
#include "bdpt_kernels.hip"

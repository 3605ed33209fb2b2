// gemm32.hip -- float instantiations of the tile engine (precision = 'single'; see gemm_kernel.hpp / gemm.hip).
#include "gemm_kernel.hpp"

int launch_gemm_f32(gpimhip_ctx* h, bool a_km, bool b_km, int epi, const GemmArgs& g) {
    return launch_gemm_t<float>(h, a_km, b_km, epi, g);
}

// the float engine's own copy of the workgroup -> tile-list map (GEMM_TILE_POS_T), on the host; quads = 1, 2, 4
int gemm_tile_pos_f32(int n, int chunk, int quads, int bx, int& quad) {
    return quads == 1 ? gemm_tile_pos_t<128, 128>(n, chunk, bx, quad)
         : quads == 2 ? gemm_tile_pos_t<64, 128>(n, chunk, bx, quad)
                      : gemm_tile_pos_t<64, 64>(n, chunk, bx, quad);
}

int gemm_shape_f32(bool a_km, bool b_km, int epi, int64_t ntiles, int64_t batch, int shape_div, int inplace) {
    if (shape_div > 1) return -1;       // (refused by launch_gemm_t)
    return gemm_shape_generic(a_km, b_km, epi, ntiles, batch, inplace);
}

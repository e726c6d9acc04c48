/*
 * mask_pairs_emul.cpp - TEST PROGRAM: tests/static_layers_emul.cpp once more, with the layer step of the compile-time table view on the
 * paired mask expanders (PAIRS = SW_PAIRS_ALL, what main_step4s of lnsfaid_kernel4s.hip instantiates) and the run-time
 * view on the single form it is compared with: all 64 lanes of every layer of the 50G-PON code, En images and rows' records equal
 * byte for byte after every layer.  Input and output as there; tests/test_mask_pairs_cpu.py drives it.
 */
#include "lnsfaid_static50.h"

template <int METHOD, int DEG, class Tab>
static inline SwRow mp_layer_step(const SwLds& lds, const Tab& tab, const SwParams& p, const SwK& K, uint32_t lane, int deg, SwRow cur, bool fresh,
                                  uint32_t rowpar, bool lme)
{
    if constexpr (SwTabStatic<Tab>::value) return sw_layer_step<METHOD, DEG, false, 1, 0, 0, SW_PAIRS_ALL>(lds, tab, p, K, lane, deg, cur, fresh, rowpar, lme);
    else return sw_layer_step<METHOD, DEG>(lds, tab, p, K, lane, deg, cur, fresh, rowpar, lme);
}
#define sw_layer_step mp_layer_step
#include "static_layers_emul.cpp"

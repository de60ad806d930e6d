// k_attn.hip - the linear self-attention block of a self_attention=True network (attn.hpp): one launch per block.
#include "host.hpp"
#include "attn.hpp"

namespace mpdx {

// what a level must look like for attn_kernel (checked by mpdx_unet_create, so that a network that cannot run is refused when it is built)
const char* attn_unsupported(int C, int L) {
    if (C < 32 || C > 512 || (C & (C - 1))) return "channels must be a power of two in [32, 512]";
    if (L < 2 || L > 128 || (L & (L - 1))) return "positions must be a power of two in [2, 128]";
    const int NC = attn_cols(C, L);
    if ((C / 16) * (NC / 16) > 4 * 16) return "channels x positions above 16384: the output accumulator does not fit the registers";
    if (attn_lds_bytes(C, L, pick_row_stride(C, CONV_S1, L, L, L)) > 160 * 1024) return "the block's working set does not fit the LDS";
    return nullptr;
}

int launch_attention(const Layer& l, AttnArgs& a, int B, hipStream_t st) {
    if (const char* why = attn_unsupported(l.cout, l.L_out)) return fail(MPDX_E_INVALID, "layer %s: %s", l.name.c_str(), why);
    a.B = B; a.L = l.L_out; a.C = l.cout;
    a.Lv = l.Lv_out > 0 ? l.Lv_out : l.L_out;
    a.NC = attn_cols(a.C, a.L); a.G = a.NC / a.L;
    a.rsx = l.rs;
    const size_t lds = attn_lds_bytes(a.C, a.L, a.rsx);
    const int tiles = (a.C / 16) * (a.NC / 16);
    auto kern = tiles <= 4 * 8 ? attn_kernel<8> : attn_kernel<16>;
    if (lds > 64 * 1024)
        if (int rc = raise_lds_limit((const void*)kern)) return rc;
    hipLaunchKernelGGL(kern, dim3((B + a.G - 1) / a.G), dim3(kAttnThreads), lds, st, a);
    return 0;
}

}  // namespace mpdx

// The elementwise halves of the recurrent cells (model/core.py:19-64: torch.nn.GRU / nn.LSTM, one layer), shared by the
// per-step kernels k_rnn_cell_fwd / k_rnn_cell_bwd (sf_rl.hip) and the row-owned sequence passes (sf_rnn.hip), so that
// a pass that fuses the time loop computes bit for bit what the per-step launches compute.  Both files are compiled
// with -ffp-contract=off: the op order below is the rounding order.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float sf_cell_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// GRU: r_pre / z_pre = gate pre-activations (x and h parts summed), xn = x W_in^T + b_in, hn = h W_hn^T + b_hn
__device__ __forceinline__ void sf_gru_cell_fwd(float r_pre, float z_pre, float xn, float hn, float hp, float &r, float &z,
                                                float &n, float &h) {
    r = sf_cell_sigmoid(r_pre);
    z = sf_cell_sigmoid(z_pre);
    n = tanhf(xn + r * hn);
    h = (1.0f - z) * n + z * hp;
}

// LSTM: the four gate pre-activations (torch order i, f, g, o) and the cell state entering the step
__device__ __forceinline__ void sf_lstm_cell_fwd(float i_pre, float f_pre, float g_pre, float o_pre, float cp, float &ig,
                                                 float &fg, float &gg, float &og, float &cn, float &h) {
    ig = sf_cell_sigmoid(i_pre);
    fg = sf_cell_sigmoid(f_pre);
    gg = tanhf(g_pre);
    og = sf_cell_sigmoid(o_pre);
    cn = fg * cp + ig * gg;
    h = og * tanhf(cn);
}

// d = dL/dh of this step (output gradient + carry).  dr, dz, dn: gradient of gx; {dr, dz, dnr = dn * r}: gradient of
// h W_hh^T + b_hh; dhd = the part of dL/dh_prev that does not go through W_hh
__device__ __forceinline__ void sf_gru_cell_bwd(float d, float r, float z, float n, float hn, float hp, float &dr, float &dz,
                                                float &dn, float &dnr, float &dhd) {
    dn = (d * (1.0f - z)) * (1.0f - n * n);
    dz = (d * (hp - n)) * (z * (1.0f - z));
    dr = (dn * hn) * (r * (1.0f - r));
    dnr = dn * r;
    dhd = d * z;
}

// dc_in = carry into c_out (0 at the last step); dcp = dL/dc_prev
__device__ __forceinline__ void sf_lstm_cell_bwd(float d, float dc_in, float ig, float fg, float gg, float og, float c_out,
                                                 float cp, float &di, float &df, float &dg, float &dob, float &dcp) {
    const float tc = tanhf(c_out);
    const float dc = d * og * (1.0f - tc * tc) + dc_in;
    di = (dc * gg) * (ig * (1.0f - ig));
    df = (dc * cp) * (fg * (1.0f - fg));
    dg = (dc * ig) * (1.0f - gg * gg);
    dob = (d * tc) * (og * (1.0f - og));
    dcp = dc * fg;
}

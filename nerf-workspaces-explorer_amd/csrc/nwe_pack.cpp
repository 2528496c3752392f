// Weight packing for both kernels (nwe_pack.h): plain C++, no HIP, so it builds and runs under host sanitizers as it is.
#include "nwe_pack.h"

#include <algorithm>
#include <cmath>

namespace nwe {
namespace {

// ---------------------------------------------------------------------------------------------
// packing for the MFMA kernel.  Must mirror nwe_mfma_eval.h (encode(), tile_mma()).
// ---------------------------------------------------------------------------------------------

// Column of gamma(v) (embedding.py:24-48 order: identity(3), then per band sin(3), cos(3)) that lane half h
// holds in element j of k-step s.  nb = bands per lane half (5 for xyz, 2 for dirs).  -1 = padding.
int gamma_col(int nb, int s, int h, int j) {
    const int q = s * 8 + j;
    if (q < 6 * nb) {
        const int pair = q >> 1, bl = pair / 3, c = pair % 3, band = bl + nb * h;
        return 3 + 6 * band + ((q & 1) ? 3 : 0) + c;
    }
    if (q == 6 * nb) return h ? 2 : 0;
    if (q == 6 * nb + 1) return h ? -1 : 1;
    return -1;
}

// Feature index that element j of k-step s holds in lane half h when a 32x32 accumulator tile is reused
// as the next B operand: tile rt = s/2, register r = 8*(s&1) + j, row = (r&3) + 8*(r>>2) + 4*h.
int hidden_col(int s, int h, int j) { return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3); }

struct Segment {
    int kind;     // 0 = hidden, 1 = gamma(x), 2 = gamma(d)
    int ksteps;
    int col_off;  // column offset of this segment in the layer's [out,in] weight
};

struct RowMap {   // which weight row feeds tile row i (or -1)
    int n_out;
    int dup4;     // 1: rows 4..7 repeat rows 0..3 (head tiles read by both lane halves)
    int operator()(int rt, int i) const {
        int r = rt * 32 + i;
        if (dup4) { if (i >= 8) return -1; r = i & 3; }
        return r < n_out ? r : -1;
    }
};

// T = float (a layer as the caller handed it over) or double (a product of two layers, see pack_mfma): the value times
// the power-of-two scale is exact in T, hi = fp16(v), lo = fp16(v - hi) with v - hi exact in T.
template <class T>
void put_tile_pair(std::vector<uint8_t>& out, const T* w, int ld, const RowMap& rows, int rt, const Segment& sg, int s, float scale) {
    const size_t base = out.size();
    out.resize(base + 2 * kTileBytes, 0);
    _Float16* hi = reinterpret_cast<_Float16*>(out.data() + base);
    _Float16* lo = reinterpret_cast<_Float16*>(out.data() + base + kTileBytes);
    for (int lane = 0; lane < 64; ++lane) {
        const int i = lane & 31, h = lane >> 5;
        const int row = rows(rt, i);
        for (int j = 0; j < 8; ++j) {
            int col = sg.kind == 0 ? hidden_col(s, h, j) : gamma_col(sg.kind == 1 ? 5 : 2, s, h, j);
            T v = 0;
            if (row >= 0 && col >= 0) v = w[(size_t)row * ld + sg.col_off + col] * (T)scale;   // power of two: exact
            const _Float16 vh = (_Float16)v;
            hi[lane * 8 + j] = vh;
            lo[lane * 8 + j] = (_Float16)(v - (T)vh);
        }
    }
}

template <class T>
void put_chunk(Packed& p, const T* w, const T* b, int ld, const RowMap& rows, int rt, const std::vector<Segment>& segs) {
    for (int i = 0; i < 32; ++i) { const int r = rows(rt, i); p.bias_tab.push_back(r >= 0 ? (float)b[r] : 0.f); }
    for (const Segment& sg : segs)
        for (int s = 0; s < sg.ksteps; ++s) put_tile_pair(p.stream, w, ld, rows, rt, sg, s, p.w_scale);
}

}  // namespace

// Stream order = the order mlp_eval() consumes chunks in.
//
// kFormFolded: _feature_linear has no activation (nerf/models/nerf_model.py:64) and its output feeds only the view layer
// (:66-70), so  W_v [W_f h + b_f ; gamma(d)] + b_v = (W_v[:, :W] W_f) h + W_v[:, W:] gamma(d) + (b_v + W_v[:, :W] b_f):
// the product is formed here in fp64 and split into (hi, lo) directly from the double, the feature layer's chunks
// disappear from the stream (8 of 78 chunks, 11 % of the MFMAs of an 8x256 evaluation).
//
// kFormNoViewDirs (use_view_dirs=False): layer D is _output_linear [out_ch, W]; its rows 0..3 (rgb_raw, sigma_raw) form the one
// chunk behind the trunk, duplicated into tile rows 4..7 for the upper lane half; further channels are ignored as the
// reference ignores them (model_utils.py:62,71).
void pack_mfma(Packed& p, const NetShape& n, int form, const float* const* w, const float* const* b) {
    const int D = n.D, W = n.W, KH = W / 16;
    const int iv = D, ife = D + 1, ia = D + 2, irgb = D + 3;
    const bool folded = form == kFormFolded, noview = form == kFormNoViewDirs;
    p.stream.clear();
    p.bias_tab.clear();
    std::vector<double> wv, bv;   // folded view layer [W/2, W + in_dir] and its bias
    if (folded) {
        const int ldv = W + n.in_dir;
        wv.assign((size_t)(W / 2) * ldv, 0.0);
        bv.assign(W / 2, 0.0);
        for (int r = 0; r < W / 2; ++r) {
            const float* vr = w[iv] + (size_t)r * ldv;
            double* o = wv.data() + (size_t)r * ldv;
            double acc_b = (double)b[iv][r];
            for (int k = 0; k < W; ++k) {
                const double vk = (double)vr[k];
                const float* fr = w[ife] + (size_t)k * W;
                for (int c = 0; c < W; ++c) o[c] += vk * (double)fr[c];
                acc_b += vk * (double)b[ife][k];
            }
            for (int c = 0; c < n.in_dir; ++c) o[W + c] = (double)vr[W + c];
            bv[r] = acc_b;
        }
    }
    // One power-of-two scale for the whole network: the largest that keeps every scaled weight below 2^14, so that
    // the lo halves (|lo| <= ulp(hi)/2) are fp16-normal for all but vanishing weights.  The kernel multiplies the
    // accumulator by 1/scale before adding the bias; both scalings are exact.
    const int in_dims[4] = {W + n.in_dir, W, W, W / 2}, out_dims[4] = {W / 2, W, 1, 3};
    double wmax = 0.0;
    for (int li = 0; li < (noview ? D + 1 : D + 4); ++li) {
        if (folded && (li == iv || li == ife || li == ia)) continue;   // folded: multiplied out / evaluated in fp32 (dot rows)
        const size_t cnt = li < D ? (size_t)W * (li == 0 ? n.in_xyz : (li == n.skip + 1 ? W + n.in_xyz : W))
                                  : (noview ? (size_t)4 * W : (size_t)in_dims[li - D] * out_dims[li - D]);
        for (size_t k = 0; k < cnt; ++k) wmax = std::max(wmax, (double)std::fabs(w[li][k]));
    }
    for (double v : wv) wmax = std::max(wmax, std::fabs(v));
    int e = 0;
    if (wmax > 0.0 && std::isfinite(wmax)) { e = 14 - (int)std::ceil(std::log2(wmax)); e = std::min(std::max(e, -14), 30); }
    p.w_scale = std::ldexp(1.f, e);
    p.colour_finite = false;
    if (folded) {
        // what the kernel multiplies with: hi = fp16(v * scale) (lo = fp16(v * scale - hi) is finite whenever hi is), fp32 biases
        bool ok = true;
        const auto fits = [&](double v) { return std::isfinite(v) && std::fabs(v * (double)p.w_scale) < 65520.0; };
        for (double v : wv) ok = ok && fits(v);
        for (double v : bv) ok = ok && std::fabs(v) <= 3.4028234663852886e38;   // NaN compares false
        for (int k = 0; k < 3 * (W / 2); ++k) ok = ok && fits((double)w[irgb][k]);
        for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(b[irgb][k]);
        p.colour_finite = ok;
    }
    auto layer = [&](int li, int n_out, int ld, int n_tiles, int dup4, const std::vector<Segment>& segs) {
        RowMap rows{n_out, dup4};
        for (int rt = 0; rt < n_tiles; ++rt) put_chunk(p, w[li], b[li], ld, rows, rt, segs);
    };
    layer(0, W, n.in_xyz, W / 32, 0, {{1, 4, 0}});
    for (int i = 1; i < D; ++i) {
        if (i == n.skip + 1) layer(i, W, W + n.in_xyz, W / 32, 0, {{1, 4, 0}, {0, KH, n.in_xyz}});   // cat([pts, h]), nerf_model.py:59
        else layer(i, W, W, W / 32, 0, {{0, KH, 0}});
    }
    if (noview) {
        layer(D, 4, W, 1, 1, {{0, KH, 0}});
        p.n_chunks = (int)(p.bias_tab.size() / 32);
        return;
    }
    if (!folded) {
        layer(ife, W, W, W / 32, 0, {{0, KH, 0}});
        layer(ia, 1, W, 1, 1, {{0, KH, 0}});
    }
    if (folded) {
        RowMap rows{W / 2, 0};
        for (int rt = 0; rt < W / 64; ++rt) put_chunk(p, wv.data(), bv.data(), W + n.in_dir, rows, rt, {{0, KH, 0}, {2, 2, W}});
    } else {
        layer(iv, W / 2, W + n.in_dir, W / 64, 0, {{0, KH, 0}, {2, 2, W}});                           // cat([feature, views]), :66
    }
    layer(irgb, 3, W / 2, 1, 1, {{0, KH / 2, 0}});
    p.n_chunks = (int)(p.bias_tab.size() / 32);
    if (folded) {
        // _alpha_linear (nerf_model.py:63) is not a tile of the folded stream: the kernel accumulates sigma = w . h + b in fp32
        // with the epilogues of the last trunk layer's tiles.  Row rt of the dot table = the weights of trunk features
        // 32 rt .. 32 rt + 31 (the row order of that layer's tile rt, like its bias row), then one row with the bias in front.
        for (int k = 0; k < W; ++k) p.bias_tab.push_back(w[ia][k]);
        p.bias_tab.push_back(b[ia][0]);
        p.bias_tab.resize(p.bias_tab.size() + 31, 0.f);
    }
}

void pack_f32(Packed& p, const NetShape& n, const float* const* w, const float* const* b) {
    p.blob.clear();
    auto add = [&](int li, int K, int N) {
        LayerF32 L; L.K = K; L.N = N; L.wt_off = (int64_t)p.blob.size();
        p.blob.resize(p.blob.size() + (size_t)K * N);
        float* wt = p.blob.data() + L.wt_off;
        for (int k = 0; k < K; ++k) for (int o = 0; o < N; ++o) wt[(size_t)k * N + o] = w[li][(size_t)o * K + k];
        L.b_off = (int64_t)p.blob.size();
        p.blob.insert(p.blob.end(), b[li], b[li] + N);
        while (p.blob.size() % 4) p.blob.push_back(0.f);
        return L;
    };
    const int D = n.D, W = n.W;
    p.f32 = {};
    p.f32.D = D; p.f32.W = W; p.f32.in_xyz = n.in_xyz; p.f32.in_dir = n.in_dir; p.f32.skip = n.skip;
    p.f32.out_ch = n.out_ch;
    p.f32.pts[0] = add(0, n.in_xyz, W);
    for (int i = 1; i < D; ++i) p.f32.pts[i] = add(i, i == n.skip + 1 ? W + n.in_xyz : W, W);
    if (n.in_dir == 0) {                    // nerf_model.py:82-83: outputs = _output_linear(h)
        p.f32.output = add(D, W, n.out_ch);
        return;
    }
    p.f32.views = add(D, W + n.in_dir, W / 2);
    p.f32.feature = add(D + 1, W, W);
    p.f32.alpha = add(D + 2, W, 1);
    p.f32.rgb = add(D + 3, W / 2, 3);
}

int64_t algo_flops(const NetShape& n) {   // 2 x MACs of nerf_model.py:53-76
    int64_t mac = (int64_t)n.in_xyz * n.W;
    for (int i = 1; i < n.D; ++i) mac += (int64_t)(i == n.skip + 1 ? n.W + n.in_xyz : n.W) * n.W;
    if (n.in_dir == 0) return 2 * (mac + (int64_t)n.W * n.out_ch);
    mac += n.W /*alpha*/ + (int64_t)n.W * n.W /*feature*/ + (int64_t)(n.W + n.in_dir) * (n.W / 2) + (int64_t)(n.W / 2) * 3;
    return 2 * mac;
}

}  // namespace nwe

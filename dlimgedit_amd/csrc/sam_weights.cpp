// SamWeights: the weight file of one SAM variant -> device-resident operands, once per GPU (sam_model.hpp).  Contract: the
// constructor runs on a stream of its own and returns with everything on the device; every value that becomes an f16 MFMA
// operand is checked against the f16 range here, so a model that loads runs; what it leaves is immutable and shared by every
// execution lane.  DLIMGEDIT_FUSED_LN=0 keeps the encoder's LayerNorms as separate kernels (A/B measurements).
#include "sam_model.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace dlimg {

namespace {

struct Loader {
    WeightFile const& file;
    hipStream_t stream;
    DeviceBuffer<float> staging;    // fp32 staging for device-side f16 conversion

    void f32(std::string const& name, std::vector<int64_t> const& dims, DeviceBuffer<float>& dst) {
        HostTensor const& t = file.get(name, dims);
        dst.reserve(t.numel());
        HIP_CHECK(hipMemcpy(dst.get(), t.data, t.numel() * 4, hipMemcpyHostToDevice));
    }
    void f32_host(std::vector<float> const& v, DeviceBuffer<float>& dst) {
        dst.reserve(v.size());
        HIP_CHECK(hipMemcpy(dst.get(), v.data(), v.size() * 4, hipMemcpyHostToDevice));
    }
    // Everything that becomes an f16 MFMA operand passes here: a value beyond the f16 range would be an infinity on the
    // device and every mask a NaN pattern, silently -- refused when the model is loaded instead (what: the tensor's name,
    // or what it was folded from)
    void f16_host(float const* src, size_t n, DeviceBuffer<half_t>& dst, std::string const& what) {
        for (size_t i = 0; i < n; ++i)
            if (!(std::fabs(src[i]) <= 65504.0f))
                throw Exception("'" + file.path() + "': " + what + " holds " + std::to_string(src[i]) + " (element " +
                                std::to_string(i) + "), outside the f16 range of this build's MFMA operands");
        staging.reserve(n);
        dst.reserve(n);
        HIP_CHECK(hipMemcpy(staging.get(), src, n * 4, hipMemcpyHostToDevice));
        k::cast_f16(staging.get(), dst.get(), n, stream);
        HIP_CHECK(hipStreamSynchronize(stream));
    }
    // head_rows / head_scale: the first head_rows output rows (weight rows and bias entries) are multiplied by head_scale
    // before anything else happens to them -- the q rows of a global-attention block's qkv (kernels.hpp, attention_global)
    void linear_h(std::string const& prefix, int out, int in, bool bias, LinearH& l, int head_rows = 0, float head_scale = 1.f) {
        HostTensor const& w = file.get(prefix + ".w", {out, in});
        if (head_rows > 0) {
            std::vector<float> ws(w.data, w.data + w.numel());
            for (size_t i = 0; i < (size_t)head_rows * in; ++i) ws[i] *= head_scale;
            f16_host(ws.data(), ws.size(), l.w, prefix + ".w");
        } else {
            f16_host(w.data, w.numel(), l.w, prefix + ".w");
        }
        l.out = out;
        l.in = in;
        l.has_bias = bias;
        if (bias && head_rows > 0) {
            HostTensor const& b = file.get(prefix + ".b", {out});
            std::vector<float> bs(b.data, b.data + out);
            for (int i = 0; i < head_rows; ++i) bs[i] *= head_scale;
            f32_host(bs, l.b);
        } else if (bias) {
            f32(prefix + ".b", {out}, l.b);
        }
    }
    // Linear layer behind a LayerNorm, with the norm folded in: y = W (g*(x-mu)*rstd + beta) + b
    //   = rstd * ((W g) x - mu * rowsum(W g)) + (b + W beta).  The GEMM multiplies the raw x by W g and applies
    // the rest per output element; rowsum is taken over the f16 values the GEMM really multiplies with.
    void linear_ln_h(std::string const& prefix, std::string const& norm, int out, int in, LinearH& l, int head_rows = 0,
                     float head_scale = 1.f) {
        HostTensor const& w = file.get(prefix + ".w", {out, in});
        HostTensor const& b = file.get(prefix + ".b", {out});
        HostTensor const& gamma = file.get(norm + ".w", {in});
        HostTensor const& beta = file.get(norm + ".b", {in});
        std::vector<float> wg((size_t)out * in), colsum(out), bias(out);
        for (int n = 0; n < out; ++n) {
            const float rs = n < head_rows ? head_scale : 1.f;      // see linear_h
            double sum = 0, shift = 0;
            for (int i = 0; i < in; ++i) {
                const float v = rs * w.data[(size_t)n * in + i] * gamma.data[i];
                wg[(size_t)n * in + i] = v;
                sum += (double)(float)(half_t)v;
                shift += (double)rs * w.data[(size_t)n * in + i] * beta.data[i];
            }
            colsum[n] = (float)sum;
            bias[n] = (float)((double)rs * b.data[n] + shift);
        }
        f16_host(wg.data(), wg.size(), l.w, prefix + ".w scaled by " + norm + ".w");
        f32_host(bias, l.b);
        f32_host(colsum, l.colsum);
        l.out = out;
        l.in = in;
        l.has_bias = true;
    }
    void linear_f(std::string const& prefix, int out, int in, LinearF& l) {
        f32(prefix + ".w", {out, in}, l.w);
        f32(prefix + ".b", {out}, l.b);
        l.out = out;
        l.in = in;
    }
    // [out][in] weight as [in][out]
    void transposed_f(std::string const& prefix, int out, int in, DeviceBuffer<float>& dst) {
        HostTensor const& w = file.get(prefix + ".w", {out, in});
        std::vector<float> t((size_t)out * in);
        for (int n = 0; n < out; ++n)
            for (int i = 0; i < in; ++i) t[(size_t)i * out + n] = w.data[(size_t)n * in + i];
        f32_host(t, dst);
    }
    void norm(std::string const& prefix, int dim, NormW& n) {
        f32(prefix + ".w", {dim}, n.w);
        f32(prefix + ".b", {dim}, n.b);
    }
    void attention(std::string const& prefix, int dim, int inner, TokenAttention& a) {
        linear_f(prefix + ".q", inner, dim, a.q);
        linear_f(prefix + ".k", inner, dim, a.k);
        linear_f(prefix + ".v", inner, dim, a.v);
        linear_f(prefix + ".o", dim, inner, a.o);
    }
    // rows of the named linears one after the other -> one f16 GEMM weight with concatenated bias
    void fused_h(std::vector<std::string> const& parts, int out_each, int in, LinearH& l) {
        const size_t n = parts.size();
        std::vector<float> w(n * (size_t)out_each * in), b(n * (size_t)out_each);
        for (size_t i = 0; i < n; ++i) {
            HostTensor const& wi = file.get(parts[i] + ".w", {out_each, in});
            HostTensor const& bi = file.get(parts[i] + ".b", {out_each});
            std::memcpy(w.data() + i * wi.numel(), wi.data, wi.numel() * 4);
            std::memcpy(b.data() + i * out_each, bi.data, bi.numel() * 4);
        }
        f16_host(w.data(), w.size(), l.w, parts[0] + ".w (fused with its siblings)");
        f32_host(b, l.b);
        l.out = int(n) * out_each;
        l.in = in;
        l.has_bias = true;
    }
    // ConvTranspose2d(k=2, s=2) weight [ci, co, 2, 2] -> GEMM weight [n = (dy*2+dx)*co_n + co][k = ci]
    void conv_transpose_h(std::string const& prefix, int ci_n, int co_n, LinearH& l) {
        HostTensor const& w = file.get(prefix + ".w", {ci_n, co_n, 2, 2});
        HostTensor const& b = file.get(prefix + ".b", {co_n});
        std::vector<float> g((size_t)4 * co_n * ci_n), gb((size_t)4 * co_n);
        for (int s = 0; s < 4; ++s)
            for (int co = 0; co < co_n; ++co) {
                gb[(size_t)s * co_n + co] = b.data[co];
                for (int ci = 0; ci < ci_n; ++ci)
                    g[((size_t)s * co_n + co) * ci_n + ci] = w.data[((size_t)ci * co_n + co) * 4 + s];
            }
        f16_host(g.data(), g.size(), l.w, prefix + ".w");
        f32_host(gb, l.b);
        l.out = 4 * co_n;
        l.in = ci_n;
        l.has_bias = true;
    }
};

}  // namespace

SamWeights::SamWeights(std::string const& weight_path, int device_index) : device(device_index) {
    WeightFile file(weight_path);
    geom_ = file.geometry();
    const int D = geom_.embed_dim, hd = geom_.head_dim();
    if (D % 64 || geom_.mlp_dim % 64) throw Exception("SAM encoder width must be a multiple of 64");
    if (D != hd * geom_.num_heads || (hd != 64 && hd != 80))
        throw Exception("SAM encoder head dimension must be 64 or 80");
    // The encoder's LayerNorms run inside the GEMMs around them (see encode()); DLIMGEDIT_FUSED_LN=0 keeps
    // them as separate kernels for A/B measurements.
    if (const char* e = std::getenv("DLIMGEDIT_FUSED_LN")) fused_ln_ = std::atoi(e) != 0;

    HIP_CHECK(hipSetDevice(device));
    hipStream_t stream_ = nullptr;
    HIP_CHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    Loader ld{file, stream_, {}};

    ld.linear_h("enc.patch", D, kPatchK, true, patch_);
    ld.f32("enc.pos", {kTokens, D}, pos_embed_);
    layers_.resize(geom_.depth);
    for (int i = 0; i < geom_.depth; ++i) {
        EncoderLayer& L = layers_[i];
        const std::string p = "enc.L" + std::to_string(i);
        L.global = geom_.is_global(i);
        const int span = L.global ? 64 : 14;
        if (!L.global) {
            HostTensor const& qb = file.get(p + ".qkv.b", {3 * D});
            ld.f16_host(qb.data, qb.numel(), L.qkv_pad, p + ".qkv.b");
        }
        // a global block's attention kernel works in units of log2 on pre-scaled operands (kernels.hpp): q rows of the
        // qkv weight and bias times log2(e) / sqrt(hd), rel-pos tables times sqrt(hd); L.qkv_pad (the windowed
        // kernel's padding bias) is not used by global blocks
        const int q_rows = L.global ? D : 0;
        const float q_scale = L.global ? k::attention_global_q_scale(hd) : 1.f;
        if (fused_ln_) {
            ld.linear_ln_h(p + ".qkv", p + ".ln1", 3 * D, D, L.qkv, q_rows, q_scale);
            ld.linear_ln_h(p + ".fc1", p + ".ln2", geom_.mlp_dim, D, L.fc1);
        } else {
            ld.norm(p + ".ln1", D, L.ln1);
            ld.norm(p + ".ln2", D, L.ln2);
            ld.linear_h(p + ".qkv", 3 * D, D, true, L.qkv, q_rows, q_scale);
            ld.linear_h(p + ".fc1", geom_.mlp_dim, D, true, L.fc1);
        }
        HostTensor const& rh = file.get(p + ".rel_h", {2 * span - 1, hd});
        HostTensor const& rw = file.get(p + ".rel_w", {2 * span - 1, hd});
        if (L.global) {
            std::vector<float> rhs(rh.data, rh.data + rh.numel()), rws(rw.data, rw.data + rw.numel());
            const float rel_scale = k::attention_global_rel_scale(hd);
            for (auto& v : rhs) v *= rel_scale;
            for (auto& v : rws) v *= rel_scale;
            ld.f16_host(rhs.data(), rhs.size(), L.rel_h16, p + ".rel_h");
            ld.f16_host(rws.data(), rws.size(), L.rel_w16, p + ".rel_w");
        } else {
            ld.f16_host(rh.data, rh.numel(), L.rel_h16, p + ".rel_h");
            ld.f16_host(rw.data, rw.numel(), L.rel_w16, p + ".rel_w");
        }
        ld.linear_h(p + ".proj", D, D, true, L.proj);
        ld.linear_h(p + ".fc2", D, geom_.mlp_dim, true, L.fc2);
    }
    ld.linear_h("enc.neck.conv1", kEmbedDim, D, false, neck1_);
    ld.norm("enc.neck.ln1", kEmbedDim, neck_ln1_);
    {   // 3x3 conv [co, ci, ky, kx] -> [co][(ky*3+kx)*256 + ci], matching im2col3x3's column order
        HostTensor const& w = file.get("enc.neck.conv2.w", {kEmbedDim, kEmbedDim, 3, 3});
        std::vector<float> g(w.numel());
        for (int co = 0; co < kEmbedDim; ++co)
            for (int ci = 0; ci < kEmbedDim; ++ci)
                for (int t = 0; t < 9; ++t)
                    g[((size_t)co * 9 + t) * kEmbedDim + ci] = w.data[((size_t)co * kEmbedDim + ci) * 9 + t];
        ld.f16_host(g.data(), g.size(), neck2_.w, "enc.neck.conv2.w");
        neck2_.out = kEmbedDim;
        neck2_.in = 9 * kEmbedDim;
    }
    ld.norm("enc.neck.ln2", kEmbedDim, neck_ln2_);
    // what the fused 3x3 launch reads for the taps that fall outside the image (k::neck_conv3x3_ln)
    zero_line_.reserve(64);
    HIP_CHECK(hipMemsetAsync(zero_line_.get(), 0, 64 * sizeof(half_t), stream_));

    DeviceBuffer<half_t> pe_h;      // dense positional encoding as a GEMM operand, only needed below
    ld.f32("pe.gauss", {2, 128}, pe_gauss_);
    ld.f32("pe.point", {4, 256}, pe_point_);
    ld.f32("pe.not_a_point", {256}, pe_not_a_point_);
    ld.f32("pe.no_mask", {256}, pe_no_mask_);
    {   // the mask branch (mask input of click-to-refine) is optional, all or nothing: a file without it serves everything but marks
        static const char* const names[] = {"pe.mask.down1.w", "pe.mask.down1.b", "pe.mask.ln1.w", "pe.mask.ln1.b", "pe.mask.down2.w",
                                            "pe.mask.down2.b", "pe.mask.ln2.w",   "pe.mask.ln2.b", "pe.mask.proj.w", "pe.mask.proj.b"};
        int present = 0;
        const char* absent = nullptr;
        for (const char* n : names) {
            if (file.has(n)) ++present;
            else absent = n;
        }
        if (present != 0 && absent)
            throw Exception("'" + file.path() + "': the mask branch pe.mask.* is all or nothing: " + std::to_string(present) +
                            " of its 10 tensors are there, '" + absent + "' is not");
        has_mask_branch_ = present != 0;
        if (has_mask_branch_) {
            ld.f32("pe.mask.down1.w", {4, 1, 2, 2}, mask_w1_);
            ld.f32("pe.mask.down1.b", {4}, mask_b1_);
            ld.norm("pe.mask.ln1", 4, mask_ln1_);
            ld.f32("pe.mask.down2.w", {16, 4, 2, 2}, mask_w2_);
            ld.f32("pe.mask.down2.b", {16}, mask_b2_);
            ld.norm("pe.mask.ln2", 16, mask_ln2_);
            ld.f32("pe.mask.proj.w", {256, 16}, mask_proj_w_);
            ld.f32("pe.mask.proj.b", {256}, mask_proj_b_);
        }
    }
    {   // dense positional encoding of the 64x64 grid (PositionEmbeddingRandom.forward), constant
        HostTensor const& g = file.get("pe.gauss", {2, 128});
        std::vector<float> pe((size_t)kTokens * 256);
        for (int y = 0; y < 64; ++y)
            for (int x = 0; x < 64; ++x) {
                const float cx = 2.0f * ((x + 0.5f) / 64.0f) - 1.0f, cy = 2.0f * ((y + 0.5f) / 64.0f) - 1.0f;
                float* row = pe.data() + ((size_t)y * 64 + x) * 256;
                for (int kf = 0; kf < 128; ++kf) {
                    const float v = 6.283185307179586f * (cx * g.data[kf] + cy * g.data[128 + kf]);
                    row[kf] = std::sin(v);
                    row[128 + kf] = std::cos(v);
                }
            }
        ld.f16_host(pe.data(), pe.size(), pe_h, "the dense positional encoding");
    }
    // (keys + pos) W = keys W + pos W: the second term is a constant of the model, computed here once (same GEMM
    // kernel, f16 pos like the sum it replaces) and added by the image-side projections as an fp32 addend.  Columns
    // past `with_pos` (the value projection, which takes the keys without pos) stay zero.
    auto pos_term = [&](LinearH const& l, int with_pos, DeviceBuffer<float>& dst) {
        dst.reserve((size_t)kTokens * l.out);
        HIP_CHECK(hipMemsetAsync(dst.get(), 0, (size_t)kTokens * l.out * sizeof(float), stream_));
        k::GemmArgs g;
        g.A = pe_h.get(); g.lda = 256; g.W = l.w.get(); g.ldw = 256;
        g.out_f32 = dst.get(); g.ldc32 = l.out; g.M = kTokens; g.N = with_pos; g.K = 256;
        SamModel::plan_inputs(g, /*shared_gpu*/ false, /*alone*/ false);     // a load has the stream to itself
        k::gemm(g, stream_);
    };
    ld.f32("dec.iou_token", {256}, iou_token_);
    ld.f32("dec.mask_tokens", {4, 256}, mask_tokens_);
    for (int i = 0; i < 2; ++i) {
        DecoderLayer& L = dec_[i];
        const std::string p = "dec.L" + std::to_string(i);
        ld.attention(p + ".self", 256, 256, L.self_attn);
        ld.norm(p + ".ln1", 256, L.ln1);
        ld.norm(p + ".ln2", 256, L.ln2);
        ld.norm(p + ".ln3", 256, L.ln3);
        ld.norm(p + ".ln4", 256, L.ln4);
        ld.linear_f(p + ".t2i.q", 128, 256, L.t2i_q);
        ld.linear_f(p + ".t2i.o", 256, 128, L.t2i_o);
        ld.transposed_f(p + ".t2i.o", 256, 128, L.t2i_o_t);
        ld.fused_h({p + ".t2i.k", p + ".i2t.q", p + ".t2i.v"}, 128, 256, L.img_kqv);
        pos_term(L.img_kqv, 256, L.pos_kqv);
        ld.linear_f(p + ".mlp.fc1", 2048, 256, L.mlp1);
        ld.linear_f(p + ".mlp.fc2", 256, 2048, L.mlp2);
        ld.linear_f(p + ".i2t.k", 128, 256, L.i2t_k);
        ld.linear_f(p + ".i2t.v", 128, 256, L.i2t_v);
        ld.linear_h(p + ".i2t.o", 256, 128, true, L.i2t_o);
    }
    ld.linear_f("dec.final.q", 128, 256, final_q_);
    ld.linear_f("dec.final.o", 256, 128, final_o_);
    ld.transposed_f("dec.final.o", 256, 128, final_o_t_);
    ld.fused_h({"dec.final.k", "dec.final.v"}, 128, 256, final_kv_);
    pos_term(final_kv_, 128, final_pos_kv_);
    ld.norm("dec.ln_final", 256, ln_final_);
    ld.conv_transpose_h("dec.up1", 256, 64, up1_);
    ld.norm("dec.up_ln", 64, up_ln_);
    ld.conv_transpose_h("dec.up2", 64, 32, up2_);
    for (int m = 0; m < 5; ++m) {
        const std::string p = m < 4 ? "dec.hyper" + std::to_string(m) : std::string("dec.iou");
        const int last = m < 4 ? 32 : 4;
        ld.linear_f(p + ".0", 256, 256, heads_[m][0]);
        ld.linear_f(p + ".1", 256, 256, heads_[m][1]);
        ld.linear_f(p + ".2", last, 256, heads_[m][2]);
    }
    {   // SAM-HQ's decoder add-on is optional, all or nothing, and independent of the mask branch
        static const char* const names[] = {
            "dec.hq.token", "dec.hq.mlp.0.w", "dec.hq.mlp.0.b", "dec.hq.mlp.1.w", "dec.hq.mlp.1.b", "dec.hq.mlp.2.w", "dec.hq.mlp.2.b",
            "dec.hq.vit.conv1.w", "dec.hq.vit.conv1.b", "dec.hq.vit.ln.w", "dec.hq.vit.ln.b", "dec.hq.vit.conv2.w", "dec.hq.vit.conv2.b",
            "dec.hq.emb.conv1.w", "dec.hq.emb.conv1.b", "dec.hq.emb.ln.w", "dec.hq.emb.ln.b", "dec.hq.emb.conv2.w", "dec.hq.emb.conv2.b",
            "dec.hq.mask.conv1.w", "dec.hq.mask.conv1.b", "dec.hq.mask.ln.w", "dec.hq.mask.ln.b", "dec.hq.mask.conv2.w", "dec.hq.mask.conv2.b"};
        int present = 0;
        const char* absent = nullptr;
        for (const char* n : names) {
            if (file.has(n)) ++present;
            else absent = n;
        }
        if (present != 0 && absent)
            throw Exception("'" + file.path() + "': the SAM-HQ group dec.hq.* is all or nothing: " + std::to_string(present) +
                            " of its 25 tensors are there, '" + absent + "' is not");
        has_hq_ = present != 0;
        if (has_hq_ && geom_.global_attn_indexes.empty())
            throw Exception("'" + file.path() + "': the SAM-HQ group needs an encoder with a global-attention block (its early feature)");
        if (has_hq_) {
            ld.f32("dec.hq.token", {256}, hq_token_);
            ld.linear_f("dec.hq.mlp.0", 256, 256, hq_mlp_[0]);
            ld.linear_f("dec.hq.mlp.1", 256, 256, hq_mlp_[1]);
            ld.linear_f("dec.hq.mlp.2", 32, 256, hq_mlp_[2]);
            ld.conv_transpose_h("dec.hq.vit.conv1", D, 256, hq_vit1_);
            ld.norm("dec.hq.vit.ln", 256, hq_vit_ln_);
            ld.conv_transpose_h("dec.hq.vit.conv2", 256, 32, hq_vit2_);
            ld.conv_transpose_h("dec.hq.emb.conv1", 256, 64, hq_emb1_);
            ld.norm("dec.hq.emb.ln", 64, hq_emb_ln_);
            ld.conv_transpose_h("dec.hq.emb.conv2", 64, 32, hq_emb2_);
            // 3x3 convolutions [co][ci][ky][kx] -> [ky * 3 + kx][co][ci], the slices the implicit GEMM of decoder_hq.hip walks
            auto conv3x3 = [&](std::string const& prefix, int co_n, int ci_n, DeviceBuffer<half_t>& w16, DeviceBuffer<float>& b) {
                HostTensor const& w = file.get(prefix + ".w", {co_n, ci_n, 3, 3});
                std::vector<float> g(w.numel());
                for (int co = 0; co < co_n; ++co)
                    for (int ci = 0; ci < ci_n; ++ci)
                        for (int t = 0; t < 9; ++t)
                            g[((size_t)t * co_n + co) * ci_n + ci] = w.data[((size_t)co * ci_n + ci) * 9 + t];
                ld.f16_host(g.data(), g.size(), w16, prefix + ".w");
                ld.f32(prefix + ".b", {co_n}, b);
            };
            conv3x3("dec.hq.mask.conv1", 64, 32, hq_conv1_w_, hq_conv1_b_);
            ld.norm("dec.hq.mask.ln", 64, hq_mask_ln_);
            conv3x3("dec.hq.mask.conv2", 32, 64, hq_conv2_w_, hq_conv2_b_);
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream_));
    HIP_CHECK(hipStreamDestroy(stream_));
}

}  // namespace dlimg

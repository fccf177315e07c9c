// dqrm_model.hip — the whole DLRM per host call: dqrm_model_fwd (inference), dqrm_model_step
// (one training step at world size 1) and dqrm_model_fwd_rowwise (inference from the row-wise
// INT4 / INT8 tables of DLRM_Net.quantize_embedding, :683-700, apply_emb :639-659), gfx950.
//
// Reference (YangZhou08/Deep_Quantized_Recommendation_Model_DQRM @ 2024-10-24): DLRM_Net.forward /
// sequential_forward (dlrm_s_pytorch_tb_dp_one_parallel_comm.py:805-880: apply_mlp(bot_l),
// apply_emb, interact_features, apply_mlp(top_l), the clamp) and one iteration of the training loop
// (loss_fn_wrap, E.backward(), the optimizer's step).
//
// dqrm_model_fwd_qact / dqrm_model_step_qact are the same two calls for a quantize_activation model
// (:475-476, :845-876): a QuantAct in front of each stack (dqrm_act_quant_fwd / _bwd) and the stacks'
// integer-activation forms (dqrm_mlp_fwd_qact / _bwd_qact), through the same bodies.
//
// There is no kernel in this file and no arithmetic: both calls validate everything first, cut the
// caller's workspace, and then call the stage exports (dqrm_emb_fwd, dqrm_mlp_fwd, dqrm_interact_*,
// dqrm_loss_fwd, dqrm_mlp_bwd, dqrm_emb_bwd_sgd[_fwd], dqrm_mlp_sgd_multi) in the order a
// stage-by-stage caller would, on the same stream. Their bits are those calls' bits by
// construction. What is saved is the host's work between the stages: one ABI crossing per step
// instead of a dozen, no autograd graph, no per-stage tensor allocation.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dqrm.h"
#include "dqrm_internal.h"

namespace {

using namespace dqrm_internal;  // set_error and the stages' checks

constexpr int64_t kMaxB = (int64_t)1 << 20;  // dqrm_loss_fwd's one workgroup
constexpr uint32_t kStepFlags = DQRM_MODEL_MLP_FRESH | DQRM_MODEL_REQUANT | DQRM_MODEL_NO_UPDATE | DQRM_MODEL_EMB_READY;
constexpr uint32_t kFwdFlags = DQRM_MODEL_MLP_FRESH | DQRM_MODEL_EMB_READY;

// the stages behind the embedding (members not null) and the widths between all of them, for T
// tables of dim D
int check_stages(const dqrm_model* m, int T, int D, const char* what) {
    int rc;
    if ((rc = check_mlp(m->bottom, what))) return rc;
    if ((rc = check_mlp(m->top, what))) return rc;
    const int Lb = m->bottom->num_layers, Lt = m->top->num_layers;
    if (Lb + Lt > DQRM_MLP_MAX_LAYERS)
        return set_error(DQRM_E_INVALID, "%s: bottom and top have %d layers in all, at most %d fit the update's launch",
                         what, Lb + Lt, DQRM_MLP_MAX_LAYERS);
    const dqrm_interact* ic = &m->interact;
    if (ic->num_features != T + 1 || ic->dim != D)
        return set_error(DQRM_E_INVALID, "%s: interact needs num_features = tables + 1 = %d and dim = %d (got %d / %d)",
                         what, T + 1, D, ic->num_features, ic->dim);
    if (ic->quant_bits != 0 && (ic->quant_bits < 2 || ic->quant_bits > 16))
        return set_error(DQRM_E_INVALID, "%s: interact.quant_bits must be 0 or 2..16 (got %d)", what, ic->quant_bits);
    const int64_t R = dqrm_interact_out_features(T + 1, D, ic->self_interaction);  // F <= 64, D % 4
    if (R < 0) return (int)R;
    const dqrm_loss* lc = m->loss;
    if (lc->kind != DQRM_LOSS_BCE && lc->kind != DQRM_LOSS_MSE && lc->kind != DQRM_LOSS_WBCE)
        return set_error(DQRM_E_INVALID, "%s: unknown loss kind %d (DQRM_LOSS_BCE / _MSE / _WBCE)", what, lc->kind);
    if (lc->kind == DQRM_LOSS_WBCE && (!lc->weights || lc->num_weights < 1))
        return set_error(DQRM_E_INVALID, "%s: DQRM_LOSS_WBCE needs weights (num_weights >= 1, got %d)", what,
                         lc->num_weights);
    if (m->bottom->layers[Lb - 1].out_features != D)
        return set_error(DQRM_E_INVALID, "%s: the bottom stack returns %d features, the tables' dim is %d", what,
                         m->bottom->layers[Lb - 1].out_features, D);
    if (m->top->layers[0].in_features != R)
        return set_error(DQRM_E_INVALID, "%s: the top stack takes %d features, the interaction returns %lld", what,
                         m->top->layers[0].in_features, (long long)R);
    if (m->top->layers[Lt - 1].out_features != 1)
        return set_error(DQRM_E_INVALID, "%s: the top stack must return 1 feature (got %d)", what,
                         m->top->layers[Lt - 1].out_features);
    return DQRM_OK;
}

// the struct alone: members, every stage's own rules, and the widths between the stages
int check_model(const dqrm_model* m, const char* what) {
    if (!m) return set_error(DQRM_E_INVALID, "%s: null model", what);
    if (!m->tables || !m->bottom || !m->top || !m->loss)
        return set_error(DQRM_E_INVALID, "%s: null tables / bottom / top / loss", what);
    int rc = emb_check(m->tables, nullptr, nullptr, m->embedding_bit, m->emb_fwd_flags, m->repack_bits, 0,
                       what);
    if (rc) return rc;
    return check_stages(m, m->tables->num_tables, m->tables->dim, what);
}

// the row-wise forward's model: `tables` may be null and is never read, the set stands in for it
int check_model_rowwise(const dqrm_model* m, const dqrm_rowwise_set* rset, const char* what) {
    if (!m) return set_error(DQRM_E_INVALID, "%s: null model", what);
    if (!m->bottom || !m->top || !m->loss)
        return set_error(DQRM_E_INVALID, "%s: null bottom / top / loss", what);
    int rc = rowwise_set_check(rset, nullptr, what);
    if (rc) return rc;
    return check_stages(m, rset->num_tables, rset->dim, what);
}

int check_B(int64_t B, const char* what) {
    if (B < 1 || B > kMaxB)
        return set_error(DQRM_E_INVALID, "%s: B must be 1..%lld (got %lld)", what, (long long)kMaxB, (long long)B);
    return DQRM_OK;
}

// the cut of the workspace: byte offsets, every part on a 256-byte boundary
struct Cut {
    size_t slab, yb[DQRM_MLP_MAX_LAYERS], r, yt[DQRM_MLP_MAX_LAYERS], dr, dx, demb;
    size_t scratch, scratch_bytes, sort, sort_bytes, iscale, rowmax, rowmax_bytes, total;
    // the quantize_activation calls only, behind everything above: the QuantActs' outputs and
    // workspaces, and the top stack's dx in front of quant_features' backward (which writes dr)
    size_t xq, rq, aws_in, aws_feat, drq;
};

size_t take(size_t& at, size_t bytes) {
    const size_t off = at;
    at += (bytes + 255) & ~(size_t)255;
    return off;
}

// model checked, B in range, max_lookups >= 0
void cut_workspace(const dqrm_model* m, int64_t B, int64_t max_lookups, Cut* c) {
    const size_t T = m->tables->num_tables, D = m->tables->dim, f = sizeof(float), b = (size_t)B;
    const size_t R = (size_t)m->top->layers[0].in_features;
    size_t at = 0;
    c->slab = take(at, b * T * D * f);
    for (int i = 0; i < m->bottom->num_layers; ++i) c->yb[i] = take(at, b * m->bottom->layers[i].out_features * f);
    c->r = take(at, b * R * f);
    for (int i = 0; i < m->top->num_layers; ++i) c->yt[i] = take(at, b * m->top->layers[i].out_features * f);
    c->dr = take(at, b * R * f);
    c->dx = take(at, b * D * f);
    c->demb = take(at, b * T * D * f);
    const size_t sb = dqrm_mlp_bwd_scratch_bytes(m->bottom, B), st = dqrm_mlp_bwd_scratch_bytes(m->top, B);
    c->scratch_bytes = sb > st ? sb : st;
    c->scratch = take(at, c->scratch_bytes);
    c->sort_bytes = dqrm_bwd_workspace_bytes((int)T, max_lookups);
    c->sort = take(at, c->sort_bytes);
    c->iscale = take(at, f);
    const dqrm_mlp* both[2] = {m->bottom, m->top};
    c->rowmax_bytes = dqrm_mlp_sgd_multi_workspace_bytes(both, 2);
    c->rowmax = take(at, c->rowmax_bytes);
    c->total = at;
}

// the quantize_activation calls' cut: dqrm_model_step's first, at its offsets
void cut_workspace_qact(const dqrm_model* m, int64_t B, int64_t max_lookups, Cut* c) {
    cut_workspace(m, B, max_lookups, c);
    const size_t f = sizeof(float), b = (size_t)B;
    const size_t X = (size_t)m->bottom->layers[0].in_features, R = (size_t)m->top->layers[0].in_features;
    size_t at = c->total;
    c->xq = take(at, b * X * f);
    c->rq = take(at, b * R * f);
    c->aws_in = take(at, (size_t)dqrm_act_quant_workspace_bytes(B * (int64_t)X));
    c->aws_feat = take(at, (size_t)dqrm_act_quant_workspace_bytes(B * (int64_t)R));
    c->drq = take(at, b * R * f);
    c->total = at;
}

int check_workspace(const Cut& c, const void* ws, size_t bytes, const char* what) {
    if (!ws || ((uintptr_t)ws & 15) || bytes < c.total)
        return set_error(DQRM_E_WORKSPACE, "%s: workspace needs %zu bytes, 16-B aligned (got %zu)", what, c.total,
                         ws ? bytes : (size_t)0);
    return DQRM_OK;
}

// everything about a call but its tensors: the model, the flags, the batches
int check_call(const dqrm_model* m, const dqrm_batch* batch, const dqrm_batch* next, uint32_t flags, uint32_t known,
               int training, const char* what) {
    int rc = check_model(m, what);
    if (rc) return rc;
    if (flags & ~known) return set_error(DQRM_E_INVALID, "%s: unknown flags 0x%x", what, flags);
    if (!batch) return set_error(DQRM_E_INVALID, "%s: null batch", what);
    if ((rc = emb_check(m->tables, batch, next, m->embedding_bit, m->emb_fwd_flags, m->repack_bits,
                        training, what)))
        return rc;
    if ((rc = check_B(batch->num_bags, what))) return rc;
    if (batch->max_lookups < 0) return set_error(DQRM_E_INVALID, "%s: negative max_lookups", what);
    // the interaction's piece index (dqrm_interact.hip's check_batch)
    if (batch->num_bags > (int64_t)INT32_MAX / ((int64_t)m->interact.num_features * (m->interact.dim / 4)))
        return set_error(DQRM_E_CAPACITY, "%s: B * num_features * dim / 4 exceeds 2^31 - 1 (B = %lld)", what,
                         (long long)batch->num_bags);
    if (next) {
        if (flags & DQRM_MODEL_NO_UPDATE)
            return set_error(DQRM_E_INVALID, "%s: a next batch needs the update (DQRM_MODEL_NO_UPDATE is set)", what);
        if (next->num_bags != batch->num_bags)
            return set_error(DQRM_E_INVALID, "%s: next has %lld bags, the slab holds %lld", what,
                             (long long)next->num_bags, (long long)batch->num_bags);
    }
    return DQRM_OK;
}

bool all_quantized(const dqrm_mlp* s, int want) {
    for (int i = 0; i < s->num_layers; ++i)
        if ((s->quantized[i] != 0) != (want != 0)) return false;
    return true;
}

// whether a quantize_activation model's stacks run the integer-activation calls (every layer
// quantized) or, full precision throughout, the plain ones behind the QuantActs (the reference's
// branch at dlrm_s_pytorch_tb_dp_one_parallel_comm.py:845-851)
bool integer_stacks(const dqrm_model* m) { return m->bottom->quantized[0] != 0; }

// the QuantAct set beside a model that passed check_model
int check_qact_set(const dqrm_model* m, const dqrm_model_qact* qa, const char* what) {
    if (!qa) return set_error(DQRM_E_INVALID, "%s: null dqrm_model_qact", what);
    int rc;
    if ((rc = check_act_quant(qa->quant_input, what))) return rc;
    if ((rc = check_act_quant(qa->quant_features, what))) return rc;
    if (all_quantized(m->bottom, 0) && all_quantized(m->top, 0)) return DQRM_OK;  // out_scale is not read
    if (!all_quantized(m->bottom, 1) || !all_quantized(m->top, 1))
        return set_error(DQRM_E_INVALID, "%s: quantized and full-precision layers are mixed: every layer of both "
                                         "stacks must be quantized, or none", what);
    if (!qa->out_scale) return set_error(DQRM_E_INVALID, "%s: null out_scale array", what);
    if ((rc = check_mlp_qact(m->bottom, qa->quant_input->scale, qa->out_scale, what))) return rc;
    return check_mlp_qact(m->top, qa->quant_features->scale, qa->out_scale + m->bottom->num_layers, what);
}

int wquant_launches(const dqrm_mlp* s) {
    int n = 0;
    for (int i = 0; i < s->num_layers; ++i)
        if (s->quantized[i]) n += s->layers[i].per_channel ? 1 : 2;
    return n;
}

// one stack's forward; qa (integer stacks): the activation scale in front and the layers' out_scales
int stack_forward(const dqrm_mlp* s, bool qa, uint32_t mf, const float* x, const float* prev, float* const* out_scale,
                  int64_t B, float* const* y, void* stream) {
    return qa ? dqrm_mlp_fwd_qact(s, mf, x, prev, out_scale, B, y, stream) : dqrm_mlp_fwd(s, mf, x, B, y, stream);
}

// the forward all calls share; g == NULL and labels == NULL as dqrm_model_fwd passes them. rset:
// the embedding stage is dqrm_rowwise_set_fwd over it, and m->tables is not read. qa: a QuantAct in
// front of each stack, writing xq / rq, which the stacks then read
int run_forward(const dqrm_model* m, const dqrm_model_qact* qa, const dqrm_rowwise_set* rset, const dqrm_interact* ic, const dqrm_batch* batch,
                uint32_t flags, const float* x, const float* labels, float* loss, float* z, float* g, char* w,
                const Cut& c, float* const* yb, float* const* yt, void* stream) {
    const int64_t B = batch->num_bags, T = ic->num_features - 1, D = ic->dim;
    const uint32_t mf = (flags & DQRM_MODEL_MLP_FRESH) ? DQRM_MLP_FRESH : 0;
    float* slab = (float*)(w + c.slab);
    float* r = (float*)(w + c.r);
    float* iscale = ic->quant_bits ? (float*)(w + c.iscale) : nullptr;
    int rc;
    if (rset) {
        if ((rc = dqrm_rowwise_set_fwd(rset, batch, nullptr, slab, D, T * D, stream))) return rc;
    } else if (!(flags & DQRM_MODEL_EMB_READY) &&
        (rc = dqrm_emb_fwd(m->tables, batch, m->embedding_bit, m->emb_fwd_flags, slab, D, T * D, stream)))
        return rc;
    const int Lb = m->bottom->num_layers;
    const bool qi = qa && integer_stacks(m);
    const float* xin = x;
    if (qa) {
        float* xq = (float*)(w + c.xq);
        if ((rc = dqrm_act_quant_fwd(qa->quant_input, x, B * m->bottom->layers[0].in_features, xq, w + c.aws_in,
                                     stream)))
            return rc;
        xin = xq;
    }
    if ((rc = stack_forward(m->bottom, qi, mf, xin, qa ? qa->quant_input->scale : nullptr, qa ? qa->out_scale : nullptr,
                            B, yb, stream)))
        return rc;
    const float* xb = yb[Lb - 1];
    if (iscale && (rc = dqrm_interact_scale(ic, xb, slab, B, iscale, stream))) return rc;
    if ((rc = dqrm_interact_fwd(ic, xb, slab, B, iscale, r, stream))) return rc;
    const float* rin = r;
    if (qa) {
        float* rq = (float*)(w + c.rq);
        if ((rc = dqrm_act_quant_fwd(qa->quant_features, r, B * m->top->layers[0].in_features, rq, w + c.aws_feat,
                                     stream)))
            return rc;
        rin = rq;
    }
    if ((rc = stack_forward(m->top, qi, mf, rin, qa ? qa->quant_features->scale : nullptr,
                            qi ? qa->out_scale + Lb : nullptr, B, yt, stream)))
        return rc;
    if (!labels) return DQRM_OK;
    return dqrm_loss_fwd(m->loss, yt[m->top->num_layers - 1], labels, B, loss, g, z, nullptr, stream);
}

void point_outputs(const dqrm_model* m, char* w, const Cut& c, float** yb, float** yt) {
    for (int i = 0; i < m->bottom->num_layers; ++i) yb[i] = (float*)(w + c.yb[i]);
    for (int i = 0; i < m->top->num_layers; ++i) yt[i] = (float*)(w + c.yt[i]);
}

dqrm_interact slab_interact(const dqrm_model* m) {
    dqrm_interact ic = m->interact;
    ic.emb_stride_b = (int64_t)(ic.num_features - 1) * ic.dim;  // the [B][T][D] slab
    ic.emb_stride_f = ic.dim;
    return ic;
}

// the row-wise forward's cut: the slab, the layers' outputs, r, the interaction's scale word and
// the per-tensor layers' row maxima; nothing of the backward (model checked, B in range)
void cut_workspace_fwd(const dqrm_model* m, int64_t B, Cut* c) {
    const size_t T = m->interact.num_features - 1, D = m->interact.dim, f = sizeof(float), b = (size_t)B;
    const size_t R = (size_t)m->top->layers[0].in_features;
    *c = Cut{};
    size_t at = 0;
    c->slab = take(at, b * T * D * f);
    for (int i = 0; i < m->bottom->num_layers; ++i) c->yb[i] = take(at, b * m->bottom->layers[i].out_features * f);
    c->r = take(at, b * R * f);
    for (int i = 0; i < m->top->num_layers; ++i) c->yt[i] = take(at, b * m->top->layers[i].out_features * f);
    c->iscale = take(at, f);
    const dqrm_mlp* both[2] = {m->bottom, m->top};
    c->rowmax_bytes = dqrm_mlp_sgd_multi_workspace_bytes(both, 2);
    c->rowmax = take(at, c->rowmax_bytes);
    c->total = at;
}

// everything about a row-wise forward but its tensors and workspace
int check_call_rowwise(const dqrm_model* m, const dqrm_rowwise_set* rset, const dqrm_batch* batch, uint32_t flags,
                       const char* what) {
    int rc = check_model_rowwise(m, rset, what);
    if (rc) return rc;
    if (flags & ~DQRM_MODEL_MLP_FRESH) return set_error(DQRM_E_INVALID, "%s: unknown flags 0x%x", what, flags);
    if (!batch) return set_error(DQRM_E_INVALID, "%s: null batch", what);
    if ((rc = rowwise_set_check(rset, batch, what))) return rc;
    if ((rc = check_B(batch->num_bags, what))) return rc;
    // the interaction's piece index (dqrm_interact.hip's check_batch)
    if (batch->num_bags > (int64_t)INT32_MAX / ((int64_t)m->interact.num_features * (m->interact.dim / 4)))
        return set_error(DQRM_E_CAPACITY, "%s: B * num_features * dim / 4 exceeds 2^31 - 1 (B = %lld)", what,
                         (long long)batch->num_bags);
    return DQRM_OK;
}

// The bodies of dqrm_model_* and dqrm_model_*_qact. qact: the quantize_activation exports, with
// their QuantAct set checked here and their longer cut; otherwise qa is not read.
int model_layout(const dqrm_model* m, const dqrm_model_qact* qa, bool qact, int64_t B, int64_t max_lookups,
                 dqrm_model_layout* out, const char* what) {
    int rc = check_model(m, what);
    if (rc) return rc;
    if (qact && (rc = check_qact_set(m, qa, what))) return rc;
    if ((rc = check_B(B, what))) return rc;
    if (max_lookups < 0) return set_error(DQRM_E_INVALID, "%s: negative max_lookups", what);
    if (!out) return set_error(DQRM_E_INVALID, "%s: null out", what);
    Cut c;
    if (qact) cut_workspace_qact(m, B, max_lookups, &c);
    else cut_workspace(m, B, max_lookups, &c);
    out->slab = c.slab;
    out->r = c.r;
    out->p = c.yt[m->top->num_layers - 1];
    out->dr = c.dr;
    out->dx = c.dx;
    out->demb = c.demb;
    out->total = c.total;
    return DQRM_OK;
}

int model_fwd(const dqrm_model* m, const dqrm_model_qact* qa, bool qact, const dqrm_batch* batch, uint32_t flags,
              const float* x, const float* labels, float* loss, float* z, void* workspace, size_t workspace_bytes,
              void* stream, const char* what) {
    int rc = check_call(m, batch, nullptr, flags, kFwdFlags, 0, what);
    if (rc) return rc;
    if (qact && (rc = check_qact_set(m, qa, what))) return rc;
    if (!x) return set_error(DQRM_E_INVALID, "%s: null x", what);
    if (labels && !loss) return set_error(DQRM_E_INVALID, "%s: labels need a loss to write (null loss)", what);
    Cut c;
    if (qact) cut_workspace_qact(m, batch->num_bags, batch->max_lookups, &c);
    else cut_workspace(m, batch->num_bags, batch->max_lookups, &c);
    if ((rc = check_workspace(c, workspace, workspace_bytes, what))) return rc;
    char* w = (char*)workspace;
    float *yb[DQRM_MLP_MAX_LAYERS], *yt[DQRM_MLP_MAX_LAYERS];
    point_outputs(m, w, c, yb, yt);
    const dqrm_interact ic = slab_interact(m);
    return run_forward(m, qact ? qa : nullptr, nullptr, &ic, batch, flags, x, labels, loss, z, nullptr, w, c, yb, yt,
                       stream);
}

int model_step(const dqrm_model* m, const dqrm_model_qact* qa, bool qact, const dqrm_batch* batch,
               const dqrm_batch* next, uint32_t flags, const float* x, const float* labels, float lr, float* loss,
               float* z, float* g, float* const* dw, float* const* db, void* workspace, size_t workspace_bytes,
               void* stream, const char* what) {
    int rc = check_call(m, batch, next, flags, kStepFlags, 1, what);
    if (rc) return rc;
    if (qact && (rc = check_qact_set(m, qa, what))) return rc;
    if (!x || !labels || !loss || !g) return set_error(DQRM_E_INVALID, "%s: null x / labels / loss / g", what);
    const int Lb = m->bottom->num_layers, Lt = m->top->num_layers;
    if (!dw || !db) return set_error(DQRM_E_INVALID, "%s: null dw / db array", what);
    for (int i = 0; i < Lb + Lt; ++i)
        if (!dw[i] || !db[i]) return set_error(DQRM_E_INVALID, "%s: null dw[%d] / db[%d]", what, i, i);
    Cut c;
    if (qact) cut_workspace_qact(m, batch->num_bags, batch->max_lookups, &c);
    else cut_workspace(m, batch->num_bags, batch->max_lookups, &c);
    if ((rc = check_workspace(c, workspace, workspace_bytes, what))) return rc;
    char* w = (char*)workspace;
    float *yb[DQRM_MLP_MAX_LAYERS], *yt[DQRM_MLP_MAX_LAYERS];
    point_outputs(m, w, c, yb, yt);
    const dqrm_interact ic = slab_interact(m);
    if (!qact) qa = nullptr;
    if ((rc = run_forward(m, qa, nullptr, &ic, batch, flags, x, labels, loss, z, g, w, c, yb, yt, stream))) return rc;

    const int64_t B = batch->num_bags, T = m->tables->num_tables, D = m->tables->dim;
    float* slab = (float*)(w + c.slab);
    float* dr = (float*)(w + c.dr);
    float* dx = (float*)(w + c.dx);
    float* demb = (float*)(w + c.demb);
    const float* iscale = ic.quant_bits ? (const float*)(w + c.iscale) : nullptr;
    void* scratch = c.scratch_bytes ? w + c.scratch : nullptr;
    // the stacks' inputs, and where the top stack's dx goes: behind a QuantAct it is that module's
    // dy, and the module's backward writes dr
    const float* xin = qa ? (const float*)(w + c.xq) : x;
    const float* rin = (const float*)(w + (qa ? c.rq : c.r));
    float* dtop = qa ? (float*)(w + c.drq) : dr;
    // loss.backward() hands the head go = 1.0, and 1.0f * g is g: the top stack's dy is g itself
    if (qa && integer_stacks(m))
        rc = dqrm_mlp_bwd_qact(m->top, rin, yt, g, qa->quant_features->scale, qa->out_scale + Lb, B, dtop, dw + Lb,
                               db + Lb, scratch, c.scratch_bytes, stream);
    else
        rc = dqrm_mlp_bwd(m->top, rin, yt, g, B, dtop, dw + Lb, db + Lb, scratch, c.scratch_bytes, stream);
    if (rc) return rc;
    if (qa && (rc = dqrm_act_quant_bwd(qa->quant_features->scale, dtop, B * m->top->layers[0].in_features, dr, stream)))
        return rc;
    if ((rc = dqrm_interact_bwd(&ic, yb[Lb - 1], slab, dr, B, iscale, dx, demb, stream))) return rc;
    // dx == NULL: nothing in front of the bottom stack takes a gradient (quant_input's input is data)
    if (qa && integer_stacks(m))
        rc = dqrm_mlp_bwd_qact(m->bottom, xin, yb, dx, qa->quant_input->scale, qa->out_scale, B, nullptr, dw, db,
                               scratch, c.scratch_bytes, stream);
    else
        rc = dqrm_mlp_bwd(m->bottom, xin, yb, dx, B, nullptr, dw, db, scratch, c.scratch_bytes, stream);
    if (rc) return rc;
    if (flags & DQRM_MODEL_NO_UPDATE) return DQRM_OK;

    void* sort = w + c.sort;
    if (next)
        rc = dqrm_emb_bwd_sgd_fwd(m->tables, batch, demb, D, T * D, m->ste, lr, m->repack_bits, sort, c.sort_bytes, next,
                                  m->embedding_bit, m->emb_fwd_flags, slab, D, T * D, stream);
    else
        rc = dqrm_emb_bwd_sgd(m->tables, batch, demb, D, T * D, m->ste, lr, m->repack_bits, sort, c.sort_bytes, stream);
    if (rc) return rc;
    const dqrm_mlp* both[2] = {m->bottom, m->top};
    return dqrm_mlp_sgd_multi(both, 2, (flags & DQRM_MODEL_REQUANT) ? DQRM_MLP_REQUANT : 0, dw, db, nullptr, lr,
                              c.rowmax_bytes ? w + c.rowmax : nullptr, c.rowmax_bytes, stream);
}

int step_launches(const dqrm_model* m, const dqrm_model_qact* qa, bool qact, const dqrm_batch* batch,
                  const dqrm_batch* next, uint32_t flags, const char* what) {
    int rc = check_call(m, batch, next, flags, kStepFlags, 1, what);
    if (rc) return rc;
    if (qact && (rc = check_qact_set(m, qa, what))) return rc;
    const int Lb = m->bottom->num_layers, Lt = m->top->num_layers;
    int n = (flags & DQRM_MODEL_EMB_READY) ? 0 : 1;                     // dqrm_emb_fwd
    n += Lb + Lt;                                                       // the stacks' forwards
    if (!(flags & DQRM_MODEL_MLP_FRESH)) n += wquant_launches(m->bottom) + wquant_launches(m->top);
    else if (qact && integer_stacks(m)) n += 2;                         // one dqrm_mlp_qact_prepare per stack
    n += (m->interact.quant_bits ? 1 : 0) + 1;                          // dqrm_interact_scale, _fwd
    n += 1;                                                             // dqrm_loss_fwd
    n += 2 * Lt + 1 + (2 * Lb - 1);                                     // top bwd, interact bwd, bottom bwd
    if (qact) {                                                         // the QuantActs' forwards, one backward
        const int64_t B = batch->num_bags;
        n += act_quant_fwd_launches(qa->quant_input, B * m->bottom->layers[0].in_features);
        n += act_quant_fwd_launches(qa->quant_features, B * m->top->layers[0].in_features) + 1;
    }
    if (flags & DQRM_MODEL_NO_UPDATE) return n;
    n += emb_bwd_sgd_launches(m->tables, batch, next, m->emb_fwd_flags);
    n += 1 + ((flags & DQRM_MODEL_REQUANT) && (has_tensor_layer(m->bottom) || has_tensor_layer(m->top)) ? 1 : 0);
    return n;
}

}  // namespace

extern "C" {

int dqrm_model_workspace_layout(const dqrm_model* m, int64_t B, int64_t max_lookups, dqrm_model_layout* out) {
    return model_layout(m, nullptr, false, B, max_lookups, out, "dqrm_model_workspace_layout");
}

size_t dqrm_model_workspace_bytes(const dqrm_model* m, int64_t B, int64_t max_lookups) {
    dqrm_model_layout l;
    return dqrm_model_workspace_layout(m, B, max_lookups, &l) ? 0 : l.total;
}

int dqrm_model_fwd(const dqrm_model* m, const dqrm_batch* batch, uint32_t flags, const float* x, const float* labels,
                   float* loss, float* z, void* workspace, size_t workspace_bytes, void* stream) {
    return model_fwd(m, nullptr, false, batch, flags, x, labels, loss, z, workspace, workspace_bytes, stream,
                     "dqrm_model_fwd");
}

int dqrm_model_step(const dqrm_model* m, const dqrm_batch* batch, const dqrm_batch* next, uint32_t flags,
                    const float* x, const float* labels, float lr, float* loss, float* z, float* g, float* const* dw,
                    float* const* db, void* workspace, size_t workspace_bytes, void* stream) {
    return model_step(m, nullptr, false, batch, next, flags, x, labels, lr, loss, z, g, dw, db, workspace,
                      workspace_bytes, stream, "dqrm_model_step");
}

int dqrm_model_step_launches(const dqrm_model* m, const dqrm_batch* batch, const dqrm_batch* next, uint32_t flags) {
    return step_launches(m, nullptr, false, batch, next, flags, "dqrm_model_step_launches");
}

int dqrm_model_qact_workspace_layout(const dqrm_model* m, const dqrm_model_qact* qa, int64_t B, int64_t max_lookups,
                                     dqrm_model_layout* out) {
    return model_layout(m, qa, true, B, max_lookups, out, "dqrm_model_qact_workspace_layout");
}

size_t dqrm_model_qact_workspace_bytes(const dqrm_model* m, const dqrm_model_qact* qa, int64_t B, int64_t max_lookups) {
    dqrm_model_layout l;
    return dqrm_model_qact_workspace_layout(m, qa, B, max_lookups, &l) ? 0 : l.total;
}

int dqrm_model_fwd_qact(const dqrm_model* m, const dqrm_model_qact* qa, const dqrm_batch* batch, uint32_t flags,
                        const float* x, const float* labels, float* loss, float* z, void* workspace,
                        size_t workspace_bytes, void* stream) {
    return model_fwd(m, qa, true, batch, flags, x, labels, loss, z, workspace, workspace_bytes, stream,
                     "dqrm_model_fwd_qact");
}

int dqrm_model_step_qact(const dqrm_model* m, const dqrm_model_qact* qa, const dqrm_batch* batch,
                         const dqrm_batch* next, uint32_t flags, const float* x, const float* labels, float lr,
                         float* loss, float* z, float* g, float* const* dw, float* const* db, void* workspace,
                         size_t workspace_bytes, void* stream) {
    return model_step(m, qa, true, batch, next, flags, x, labels, lr, loss, z, g, dw, db, workspace, workspace_bytes,
                      stream, "dqrm_model_step_qact");
}

int dqrm_model_qact_step_launches(const dqrm_model* m, const dqrm_model_qact* qa, const dqrm_batch* batch,
                                  const dqrm_batch* next, uint32_t flags) {
    return step_launches(m, qa, true, batch, next, flags, "dqrm_model_qact_step_launches");
}

int dqrm_model_fwd_rowwise_workspace_layout(const dqrm_model* m, const dqrm_rowwise_set* rset, int64_t B,
                                            dqrm_model_layout* out) {
    const char* what = "dqrm_model_fwd_rowwise_workspace_layout";
    int rc = check_model_rowwise(m, rset, what);
    if (rc) return rc;
    if ((rc = check_B(B, what))) return rc;
    if (!out) return set_error(DQRM_E_INVALID, "%s: null out", what);
    Cut c;
    cut_workspace_fwd(m, B, &c);
    *out = dqrm_model_layout{};
    out->slab = c.slab;
    out->r = c.r;
    out->p = c.yt[m->top->num_layers - 1];
    out->total = c.total;
    return DQRM_OK;
}

size_t dqrm_model_fwd_rowwise_workspace_bytes(const dqrm_model* m, const dqrm_rowwise_set* rset, int64_t B) {
    dqrm_model_layout l;
    return dqrm_model_fwd_rowwise_workspace_layout(m, rset, B, &l) ? 0 : l.total;
}

int dqrm_model_fwd_rowwise(const dqrm_model* m, const dqrm_rowwise_set* rset, const dqrm_batch* batch, uint32_t flags,
                           const float* x, const float* labels, float* loss, float* z, void* workspace,
                           size_t workspace_bytes, void* stream) {
    const char* what = "dqrm_model_fwd_rowwise";
    int rc = check_call_rowwise(m, rset, batch, flags, what);
    if (rc) return rc;
    if (!x) return set_error(DQRM_E_INVALID, "%s: null x", what);
    if (labels && !loss) return set_error(DQRM_E_INVALID, "%s: labels need a loss to write (null loss)", what);
    Cut c;
    cut_workspace_fwd(m, batch->num_bags, &c);
    if ((rc = check_workspace(c, workspace, workspace_bytes, what))) return rc;
    char* w = (char*)workspace;
    float *yb[DQRM_MLP_MAX_LAYERS], *yt[DQRM_MLP_MAX_LAYERS];
    point_outputs(m, w, c, yb, yt);
    const dqrm_interact ic = slab_interact(m);
    return run_forward(m, nullptr, rset, &ic, batch, flags, x, labels, loss, z, nullptr, w, c, yb, yt, stream);
}

int dqrm_model_fwd_rowwise_launches(const dqrm_model* m, const dqrm_rowwise_set* rset, const dqrm_batch* batch,
                                    uint32_t flags, int has_labels) {
    const char* what = "dqrm_model_fwd_rowwise_launches";
    int rc = check_call_rowwise(m, rset, batch, flags, what);
    if (rc) return rc;
    int n = 1;                                                          // dqrm_rowwise_set_fwd
    n += m->bottom->num_layers + m->top->num_layers;                    // the stacks' forwards
    if (!(flags & DQRM_MODEL_MLP_FRESH)) n += wquant_launches(m->bottom) + wquant_launches(m->top);
    n += (m->interact.quant_bits ? 1 : 0) + 1;                          // dqrm_interact_scale, _fwd
    n += has_labels ? 1 : 0;                                            // dqrm_loss_fwd
    return n;
}

}  // extern "C"

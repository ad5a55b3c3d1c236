/* oracle_scenegraph.c — TEST INFRASTRUCTURE ONLY: a plain-C restatement of the reference's Scene::UpdateSceneGraph without the BLAS / TLAS builds, written from
 * tiny_scene.h's text and SEQUENTIALLY, as the reference runs: Animation::Update -> Channel::Update -> Sampler::SampleVec3 / SampleQuat / SampleFloat (2457-2626),
 * ts_quat::slerp and ts_normalize (962-982, 304-305), Node::UpdateTransformFromTRS (1939-1951), the recursive Node::Update (1959-1990, 2129-2138) with ts_invert
 * (886-911) and the skins' joint matrices computed where the recursion computes them.  It shares nothing with tinybvh_amd/csrc/scenegraph.h: no flat work items,
 * no shadowed channels (later channels simply overwrite), no table of stale joints (a joint visited later IS last walk's matrix here), no ancestor lists.  The
 * fused multiply-adds of the reference's build (g++ -O3 -mavx2 -mfma; DESIGN.md par. 17) are spelled out; built -ffp-contract=off.
 * sgorc_slerp / sgorc_slerp_spread evaluate slerp's trigonometric branch with each of its four libm results moved by a number of ulps: the tolerance of that
 * branch is derived from them. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "tinybvh_amd.h"   /* the descriptor and the download codes only */

static float ulps(float x, int n) {
    for (; n > 0; n--) x = nextafterf(x, INFINITY);
    for (; n < 0; n++) x = nextafterf(x, -INFINITY);
    return x;
}

/* a, b: w x y z; d[0..3]: ulps added to acosf( cosTheta ), sinf( (1 - t) * angle ), sinf( t * angle ), sinf( angle ).  out: the normalised quaternion.
 * Returns 1 when the trigonometric branch was taken, 0 for the lerp branch (d is then not used). */
int sgorc_slerp(const float* a, const float* b, float t, const int* d, float* out) {
    float r[4] = {b[0], b[1], b[2], b[3]};
    float c = fmaf(a[3], r[3], fmaf(a[2], r[2], fmaf(a[0], r[0], a[1] * r[1])));
    int trig = 0, i;
    if (c < 0) { for (i = 0; i < 4; i++) r[i] = r[i] * -1.0f; c = -c; }
    if (c > 0.99f) {
        for (i = 0; i < 4; i++) r[i] = fmaf(t, r[i], (1 - t) * a[i]);
    } else {
        const float angle = ulps(acosf(c), d[0]);
        const float s1 = ulps(sinf((1 - t) * angle), d[1]), s2 = ulps(sinf(t * angle), d[2]), rs3 = 1.0f / ulps(sinf(angle), d[3]);
        for (i = 0; i < 4; i++) r[i] = fmaf(s1, a[i], s2 * r[i]) * rs3;
        trig = 1;
    }
    {
        const float m = sqrtf(fmaf(r[3], r[3], fmaf(r[2], r[2], fmaf(r[0], r[0], r[1] * r[1]))));
        const float s = 1 / m;
        for (i = 0; i < 4; i++) out[i] = r[i] * s;
    }
    return trig;
}

/* the largest |component| difference between sgorc_slerp with every combination of d[i] in { -u, 0, +u } and `want` (the real reference's result) */
float sgorc_slerp_spread(const float* a, const float* b, float t, int u, const float* want) {
    float worst = 0, q[4];
    int d[4], n, i;
    for (n = 0; n < 81; n++) {
        int m = n;
        for (i = 0; i < 4; i++) { d[i] = (m % 3 - 1) * u; m /= 3; }
        sgorc_slerp(a, b, t, d, q);
        for (i = 0; i < 4; i++) { const float e = fabsf(q[i] - want[i]); if (e > worst || e != e) worst = e; }
    }
    return worst;
}

/* ---- the whole graph ------------------------------------------------------------------------------------------------------------------------ */
typedef struct {
    float translation[3], rotation[4] /* w x y z */, scale[3], matrix[16], localTransform[16], combinedTransform[16];
    int transformed, nChildren, skin, firstWeight, nWeights;
    int* childIdx;
} Node;
typedef struct { int samplerIdx, nodeIdx, target, animation, k; float t; } Channel;
typedef struct { int interpolation, type, keyCount, nValues; const float *t, *v; } Sampler;
typedef struct { int meshNode, first, count; } Skin;
typedef struct {
    int nNodes, nRoots, nSamplers, nChannels, nInstances, nSkins, nJoints, nWeightsTotal, fresh;
    Node* nodes; int* roots; Sampler* samplers; Channel* channels; float *times, *values, *weights; int* instNode; Skin* skins; int* jointNode;
    float *inverseBind, *jointMat, *instTransform;
} Graph;

static void identity(float* m) { int i; for (i = 0; i < 16; i++) m[i] = (i % 5) == 0 ? 1.f : 0.f; }

/* bvhmat4 operator*: (a0*b0) + (a1*b4) + (a2*b8) + (a3*b12) */
static void mul(const float* a, const float* b, float* r) {
    int i, j;
    for (i = 0; i < 16; i += 4) for (j = 0; j < 4; j++)
        r[i + j] = fmaf(a[i + 3], b[j + 12], fmaf(a[i + 2], b[j + 8], fmaf(a[i + 0], b[j + 0], a[i + 1] * b[j + 4])));
}

/* ts_invert: the MESA cofactor table; rows are { sign, first, second, third factor } of the six terms of each cell, in the order the text has them */
static const signed char COF[16][6][4] = {
    {{1, 5, 10, 15}, {-1, 5, 11, 14}, {-1, 9, 6, 15}, {1, 9, 7, 14}, {1, 13, 6, 11}, {-1, 13, 7, 10}},
    {{-1, 1, 10, 15}, {1, 1, 11, 14}, {1, 9, 2, 15}, {-1, 9, 3, 14}, {-1, 13, 2, 11}, {1, 13, 3, 10}},
    {{1, 1, 6, 15}, {-1, 1, 7, 14}, {-1, 5, 2, 15}, {1, 5, 3, 14}, {1, 13, 2, 7}, {-1, 13, 3, 6}},
    {{-1, 1, 6, 11}, {1, 1, 7, 10}, {1, 5, 2, 11}, {-1, 5, 3, 10}, {-1, 9, 2, 7}, {1, 9, 3, 6}},
    {{-1, 4, 10, 15}, {1, 4, 11, 14}, {1, 8, 6, 15}, {-1, 8, 7, 14}, {-1, 12, 6, 11}, {1, 12, 7, 10}},
    {{1, 0, 10, 15}, {-1, 0, 11, 14}, {-1, 8, 2, 15}, {1, 8, 3, 14}, {1, 12, 2, 11}, {-1, 12, 3, 10}},
    {{-1, 0, 6, 15}, {1, 0, 7, 14}, {1, 4, 2, 15}, {-1, 4, 3, 14}, {-1, 12, 2, 7}, {1, 12, 3, 6}},
    {{1, 0, 6, 11}, {-1, 0, 7, 10}, {-1, 4, 2, 11}, {1, 4, 3, 10}, {1, 8, 2, 7}, {-1, 8, 3, 6}},
    {{1, 4, 9, 15}, {-1, 4, 11, 13}, {-1, 8, 5, 15}, {1, 8, 7, 13}, {1, 12, 5, 11}, {-1, 12, 7, 9}},
    {{-1, 0, 9, 15}, {1, 0, 11, 13}, {1, 8, 1, 15}, {-1, 8, 3, 13}, {-1, 12, 1, 11}, {1, 12, 3, 9}},
    {{1, 0, 5, 15}, {-1, 0, 7, 13}, {-1, 4, 1, 15}, {1, 4, 3, 13}, {1, 12, 1, 7}, {-1, 12, 3, 5}},
    {{-1, 0, 5, 11}, {1, 0, 7, 9}, {1, 4, 1, 11}, {-1, 4, 3, 9}, {-1, 8, 1, 7}, {1, 8, 3, 5}},
    {{-1, 4, 9, 14}, {1, 4, 10, 13}, {1, 8, 5, 14}, {-1, 8, 6, 13}, {-1, 12, 5, 10}, {1, 12, 6, 9}},
    {{1, 0, 9, 14}, {-1, 0, 10, 13}, {-1, 8, 1, 14}, {1, 8, 2, 13}, {1, 12, 1, 10}, {-1, 12, 2, 9}},
    {{-1, 0, 5, 14}, {1, 0, 6, 13}, {1, 4, 1, 14}, {-1, 4, 2, 13}, {-1, 12, 1, 6}, {1, 12, 2, 5}},
    {{1, 0, 5, 10}, {-1, 0, 6, 9}, {-1, 4, 1, 10}, {1, 4, 2, 9}, {1, 8, 1, 6}, {-1, 8, 2, 5}}};

static void invert(float* T) {
    float inv[16], det, invdet;
    int c, k, i;
    for (c = 0; c < 16; c++) {
        /* the first term is rounded ( (a * b) * c ), every later one is fused onto the sum with its sign */
        float r = ((float)COF[c][0][0] * T[COF[c][0][1]]) * T[COF[c][0][2]] * T[COF[c][0][3]];
        for (k = 1; k < 6; k++) r = fmaf((float)COF[c][k][0] * (T[COF[c][k][1]] * T[COF[c][k][2]]), T[COF[c][k][3]], r);
        inv[c] = r;
    }
    det = fmaf(T[3], inv[12], fmaf(T[2], inv[8], fmaf(T[0], inv[0], T[1] * inv[4])));
    if (det == 0) return;
    invdet = 1.0f / det;
    for (i = 0; i < 16; i++) T[i] = inv[i] * invdet;
}

static void updateTransformFromTRS(Node* n) {
    float T[16], R[16], S[16], a[16], b[16];
    const float rw = n->rotation[0], rx = n->rotation[1], ry = n->rotation[2], rz = n->rotation[3];
    identity(T); identity(R); identity(S);
    T[3] = n->translation[0]; T[7] = n->translation[1]; T[11] = n->translation[2];
    R[0] = fmaf(-(2 * rz), rz, fmaf(-(2 * ry), ry, 1.f)); R[1] = fmaf(2 * rx, ry, -(2 * rw * rz));
    R[2] = fmaf(2 * rx, rz, 2 * rw * ry); R[4] = fmaf(2 * rx, ry, 2 * rw * rz);
    R[5] = fmaf(-(2 * rz), rz, fmaf(-(2 * rx), rx, 1.f)); R[6] = fmaf(2 * ry, rz, -(2 * rw * rx));
    R[8] = fmaf(2 * rx, rz, -(2 * rw * ry)); R[9] = fmaf(2 * ry, rz, 2 * rw * rx);
    R[10] = fmaf(-(2 * ry), ry, fmaf(-(2 * rx), rx, 1.f));
    S[0] = n->scale[0]; S[5] = n->scale[1]; S[10] = n->scale[2];
    mul(T, R, a); mul(a, S, b); mul(b, n->matrix, n->localTransform);
}

static void jointMatrices(Graph* g, const Node* n) {
    float invTransform[16], a[16];
    const Skin* skin = &g->skins[n->skin];
    int j;
    memcpy(invTransform, n->combinedTransform, 64);
    invert(invTransform);
    for (j = 0; j < skin->count; j++) {
        mul(invTransform, g->nodes[g->jointNode[skin->first + j]].combinedTransform, a);
        mul(a, g->inverseBind + 16 * (size_t)(skin->first + j), g->jointMat + 16 * (size_t)(skin->first + j));
    }
}

static void nodeUpdate(Graph* g, Node* n, const float* T) {
    int i;
    if (n->transformed) updateTransformFromTRS(n);
    mul(T, n->localTransform, n->combinedTransform);
    for (i = 0; i < n->nChildren; i++) nodeUpdate(g, &g->nodes[n->childIdx[i]], n->combinedTransform);
    if (n->skin >= 0) jointMatrices(g, n);
    n->transformed = 0;
}

static void spline4(float tt, float* c) {
    const float t2 = tt * tt, t3 = t2 * tt;
    c[0] = fmaf(-2.f, t2, t3) + tt; c[1] = fmaf(2.f, t3, -(3 * t2)) + 1; c[2] = fmaf(-2.f, t3, 3 * t2); c[3] = t3 - t2;
}

static void normalize4(float* q) {
    const float m = sqrtf(fmaf(q[3], q[3], fmaf(q[2], q[2], fmaf(q[0], q[0], q[1] * q[1]))));
    const float s = 1 / m;
    int i;
    for (i = 0; i < 4; i++) q[i] = q[i] * s;
}

/* SampleVec3 (W = 3) and SampleQuat (W = 4) */
static void sampleVec(const Sampler* s, int W, float currentTime, int k, float* out) {
    const float* key = s->v;
    float t0, t1, f, c[4];
    int i;
    if (k == 0 && currentTime < s->t[0]) { memcpy(out, key + (s->interpolation == TBVH_GRAPH_SPLINE ? W : 0), 4 * W); return; }
    t0 = s->t[k]; t1 = s->t[k + 1];
    f = (currentTime - t0) / (t1 - t0);
    if (f <= 0) { memcpy(out, key, 4 * W); return; }
    switch (s->interpolation) {
    case TBVH_GRAPH_SPLINE: {
        const float *p0 = key + (k * 3 + 1) * W, *m0 = key + (k * 3 + 2) * W, *p1 = key + ((k + 1) * 3 + 1) * W, *m1 = key + ((k + 1) * 3) * W;
        spline4(f, c);
        for (i = 0; i < W; i++) out[i] = fmaf((t1 - t0) * m1[i], c[3], fmaf(p1[i], c[2], fmaf(p0[i], c[1], ((t1 - t0) * m0[i]) * c[0])));
        if (W == 4) normalize4(out);
        return;
    }
    case TBVH_GRAPH_STEP: memcpy(out, key + k * W, 4 * W); return;
    default:
        if (W == 3) for (i = 0; i < 3; i++) out[i] = fmaf(f, key[(k + 1) * 3 + i], (1 - f) * key[k * 3 + i]);
        else { const int zero[4] = {0, 0, 0, 0}; sgorc_slerp(key + k * 4, key + (k + 1) * 4, f, zero, out); }   /* (normalises) */
    }
}

static float sampleFloat(const Sampler* s, float currentTime, int k, int i, int count) {
    const float* floatKey = s->v;
    float t0, t1, f, c[4];
    if (k == 0 && currentTime < s->t[0]) return s->interpolation == TBVH_GRAPH_SPLINE ? floatKey[1] : floatKey[0];
    t0 = s->t[k]; t1 = s->t[k + 1];
    f = (currentTime - t0) / (t1 - t0);
    if (f <= 0) return floatKey[0];
    switch (s->interpolation) {
    case TBVH_GRAPH_SPLINE: {
        const float p0 = floatKey[(k * count + i) * 3 + 1], m0 = (t1 - t0) * floatKey[(k * count + i) * 3 + 2];
        const float p1 = floatKey[((k + 1) * count + i) * 3 + 1], m1 = (t1 - t0) * floatKey[((k + 1) * count + i) * 3];
        spline4(f, c);
        return fmaf(m1, c[3], fmaf(p1, c[2], fmaf(m0, c[0], p0 * c[1])));
    }
    case TBVH_GRAPH_STEP: return floatKey[k];
    default: return fmaf(1 - f, floatKey[k * count + i], f * floatKey[(k + 1) * count + i]);
    }
}

static void channelUpdate(Graph* g, Channel* ch, float dt) {
    const Sampler* sampler = &g->samplers[ch->samplerIdx];
    Node* node = &g->nodes[ch->nodeIdx];
    const int keyCount = sampler->keyCount;
    const float animDuration = sampler->t[keyCount - 1];
    int i;
    ch->t += dt;
    if (animDuration == 0 || keyCount == 1) {
        if (ch->target == 0) { memcpy(node->translation, sampler->v, 12); node->transformed = 1; }
        else if (ch->target == 1) { memcpy(node->rotation, sampler->v, 16); node->transformed = 1; }
        else if (ch->target == 2) { memcpy(node->scale, sampler->v, 12); node->transformed = 1; }
        else for (i = 0; i < node->nWeights; i++) g->weights[node->firstWeight + i] = sampler->v[0];
    } else {
        while (ch->t >= animDuration) ch->t -= animDuration, ch->k = 0;
        while (ch->t >= sampler->t[(ch->k + 1) % keyCount]) ch->k++;
        if (ch->target == 0) { sampleVec(sampler, 3, ch->t, ch->k, node->translation); node->transformed = 1; }
        else if (ch->target == 1) { sampleVec(sampler, 4, ch->t, ch->k, node->rotation); node->transformed = 1; }
        else if (ch->target == 2) { sampleVec(sampler, 3, ch->t, ch->k, node->scale); node->transformed = 1; }
        else for (i = 0; i < node->nWeights; i++) g->weights[node->firstWeight + i] = sampleFloat(sampler, ch->t, ch->k, i, node->nWeights);
    }
}

static void* copyOf(const void* p, size_t bytes) { void* q = malloc(bytes ? bytes : 1); if (bytes) memcpy(q, p, bytes); return q; }

/* the descriptor is taken as valid (the library's own creation call has accepted it) */
void* sgorc_create(const tbvh_scenegraph_desc* d) {
    Graph* g = (Graph*)calloc(1, sizeof(Graph));
    int n, i, c, u;
    int* count;
    g->nNodes = (int)d->n_nodes; g->nSamplers = (int)d->n_samplers; g->nChannels = (int)d->n_channels; g->nInstances = (int)d->n_instances; g->nSkins = (int)d->n_skin_uses;
    g->fresh = (d->flags & TBVH_SCENEGRAPH_FRESH_JOINTS) != 0;
    g->nodes = (Node*)calloc(g->nNodes, sizeof(Node));
    g->roots = (int*)malloc(sizeof(int) * g->nNodes);
    count = (int*)calloc(g->nNodes, sizeof(int));
    for (n = 0; n < g->nNodes; n++) {
        Node* nd = &g->nodes[n];
        memcpy(nd->translation, d->translation + 3 * n, 12); memcpy(nd->rotation, d->rotation + 4 * n, 16); memcpy(nd->scale, d->scale + 3 * n, 12);
        memcpy(nd->matrix, d->matrix + 16 * n, 64); memcpy(nd->localTransform, d->local_transform + 16 * n, 64);
        identity(nd->combinedTransform);
        nd->skin = -1; nd->firstWeight = g->nWeightsTotal; nd->nWeights = d->n_weights ? (int)d->n_weights[n] : 0;
        g->nWeightsTotal += nd->nWeights;
        if (d->parent[n] >= 0) count[d->parent[n]]++;
    }
    for (n = 0; n < g->nNodes; n++) g->nodes[n].childIdx = (int*)malloc(sizeof(int) * (count[n] ? count[n] : 1));
    for (i = 0; i < g->nNodes; i++) {   /* children and roots in the walk's order */
        n = d->visit_order ? (int)d->visit_order[i] : i;
        if (d->parent[n] < 0) g->roots[g->nRoots++] = n;
        else { Node* p = &g->nodes[d->parent[n]]; p->childIdx[p->nChildren++] = n; }
    }
    free(count);
    g->weights = (float*)calloc(g->nWeightsTotal ? g->nWeightsTotal : 1, 4);
    if (d->weights && g->nWeightsTotal) memcpy(g->weights, d->weights, 4 * (size_t)g->nWeightsTotal);
    g->times = (float*)copyOf(d->key_times, g->nSamplers ? 4 * (size_t)d->sampler_key_offset[g->nSamplers] : 0);
    g->values = (float*)copyOf(d->key_values, g->nSamplers ? 4 * (size_t)d->sampler_value_offset[g->nSamplers] : 0);
    g->samplers = (Sampler*)calloc(g->nSamplers ? g->nSamplers : 1, sizeof(Sampler));
    for (i = 0; i < g->nSamplers; i++) {
        Sampler* s = &g->samplers[i];
        s->interpolation = (int)d->sampler_interpolation[i]; s->type = (int)d->sampler_type[i];
        s->keyCount = (int)(d->sampler_key_offset[i + 1] - d->sampler_key_offset[i]); s->nValues = (int)(d->sampler_value_offset[i + 1] - d->sampler_value_offset[i]);
        s->t = g->times + d->sampler_key_offset[i]; s->v = g->values + d->sampler_value_offset[i];
    }
    g->channels = (Channel*)calloc(g->nChannels ? g->nChannels : 1, sizeof(Channel));
    for (c = 0; c < g->nChannels; c++) {
        Channel* ch = &g->channels[c];
        ch->animation = (int)d->channel_animation[c]; ch->samplerIdx = (int)d->channel_sampler[c]; ch->nodeIdx = (int)d->channel_node[c]; ch->target = (int)d->channel_target[c];
    }
    g->instNode = (int*)copyOf(d->node_of_instance, 4 * (size_t)g->nInstances);
    g->instTransform = (float*)calloc((size_t)(g->nInstances ? g->nInstances : 1) * 16, 4);
    g->skins = (Skin*)calloc(g->nSkins ? g->nSkins : 1, sizeof(Skin));
    g->nJoints = g->nSkins ? (int)d->skin_joint_offset[g->nSkins] : 0;
    for (u = 0; u < g->nSkins; u++) {
        g->skins[u].meshNode = (int)d->skin_mesh_node[u]; g->skins[u].first = (int)d->skin_joint_offset[u];
        g->skins[u].count = (int)(d->skin_joint_offset[u + 1] - d->skin_joint_offset[u]);
        g->nodes[g->skins[u].meshNode].skin = u;
    }
    g->jointNode = (int*)copyOf(d->skin_joint_node, 4 * (size_t)g->nJoints);
    g->inverseBind = (float*)copyOf(d->skin_inverse_bind, 64 * (size_t)g->nJoints);
    g->jointMat = (float*)calloc((size_t)(g->nJoints ? g->nJoints : 1) * 16, 4);
    return g;
}

void sgorc_free(void* h) {
    Graph* g = (Graph*)h;
    int n;
    for (n = 0; n < g->nNodes; n++) free(g->nodes[n].childIdx);
    free(g->nodes); free(g->roots); free(g->samplers); free(g->channels); free(g->times); free(g->values); free(g->weights); free(g->instNode); free(g->skins);
    free(g->jointNode); free(g->inverseBind); free(g->jointMat); free(g->instTransform); free(g);
}

void sgorc_advance_animation(void* h, uint32_t a, float dt) {
    Graph* g = (Graph*)h;
    int c;
    for (c = 0; c < g->nChannels; c++) if (g->channels[c].animation == (int)a) channelUpdate(g, &g->channels[c], dt);
}

void sgorc_update_nodes(void* h) {
    Graph* g = (Graph*)h;
    float T[16];
    int r, i, u;
    for (r = 0; r < g->nRoots; r++) { identity(T); nodeUpdate(g, &g->nodes[g->roots[r]], T); }
    for (i = 0; i < g->nInstances; i++) memcpy(g->instTransform + 16 * (size_t)i, g->nodes[g->instNode[i]].combinedTransform, 64);
    if (g->fresh) for (u = 0; u < g->nSkins; u++) jointMatrices(g, &g->nodes[g->skins[u].meshNode]);   /* the library's option: every joint from THIS walk */
}

void sgorc_advance(void* h, float dt) {
    Graph* g = (Graph*)h;
    int c;
    for (c = 0; c < g->nChannels; c++) channelUpdate(g, &g->channels[c], dt);   /* (the channels are sorted by animation: UpdateAnimation( 0 ), ( 1 ), ... ) */
    sgorc_update_nodes(h);
}

void sgorc_set_time(void* h, uint32_t a, float t) {
    Graph* g = (Graph*)h;
    int c;
    for (c = 0; c < g->nChannels; c++) if (g->channels[c].animation == (int)a) { g->channels[c].t = t; g->channels[c].k = 0; }
}
void sgorc_reset(void* h, uint32_t a) { sgorc_set_time(h, a, 0.f); }
void sgorc_set_local(void* h, uint32_t node, const float* m) { memcpy(((Graph*)h)->nodes[node].localTransform, m, 64); }
/* every node's T, R, S replaced (10 floats each: translation, rotation w x y z, scale); the `transformed` marks stay */
void sgorc_set_trs(void* h, const float* trs) {
    Graph* g = (Graph*)h;
    int n;
    for (n = 0; n < g->nNodes; n++) { memcpy(g->nodes[n].translation, trs + 10 * n, 12); memcpy(g->nodes[n].rotation, trs + 10 * n + 3, 16); memcpy(g->nodes[n].scale, trs + 10 * n + 7, 12); }
}

int sgorc_download(void* h, int what, void* dst) {
    Graph* g = (Graph*)h;
    float* f = (float*)dst;
    int n, c;
    switch (what) {
    case TBVH_GRAPH_TRS: for (n = 0; n < g->nNodes; n++) { memcpy(f + 10 * n, g->nodes[n].translation, 12); memcpy(f + 10 * n + 3, g->nodes[n].rotation, 16); memcpy(f + 10 * n + 7, g->nodes[n].scale, 12); } return 0;
    case TBVH_GRAPH_LOCAL: for (n = 0; n < g->nNodes; n++) memcpy(f + 16 * n, g->nodes[n].localTransform, 64); return 0;
    case TBVH_GRAPH_COMBINED: for (n = 0; n < g->nNodes; n++) memcpy(f + 16 * n, g->nodes[n].combinedTransform, 64); return 0;
    case TBVH_GRAPH_CHANNEL_T: for (c = 0; c < g->nChannels; c++) f[c] = g->channels[c].t; return 0;
    case TBVH_GRAPH_CHANNEL_K: for (c = 0; c < g->nChannels; c++) ((int32_t*)dst)[c] = g->channels[c].k; return 0;
    case TBVH_GRAPH_INSTANCES: memcpy(dst, g->instTransform, 64 * (size_t)g->nInstances); return 0;
    case TBVH_GRAPH_JOINTS: memcpy(dst, g->jointMat, 64 * (size_t)g->nJoints); return 0;
    case TBVH_GRAPH_WEIGHTS: memcpy(dst, g->weights, 4 * (size_t)g->nWeightsTotal); return 0;
    }
    return -1;
}

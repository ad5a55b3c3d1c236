/* tinybvh_amd_debug.h — development aids of the MI355X engine: instrumentation counters, experiment switches, forced kernel schedules, the
 * coherence probe's last verdict.  NOT part of the boundary a tinybvh maintainer binds (include/tinybvh_amd.h is); used by tests/ and tools/.
 * Same library, same ABI version. */
#ifndef TINYBVH_AMD_DEBUG_H_
#define TINYBVH_AMD_DEBUG_H_
#include "tinybvh_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Lane-utilisation counters of the instrumented kernel variants (development aid):
 * out[0] wave iterations, [1] sum of active lanes, [2] sum of lanes in the node step,
 * [3] triangle-loop iterations, [4] sum of lanes in them, [5] refill events, [6] rays handed out. */
int tbvh_debug_stats(tbvh_context* ctx, uint64_t out[8], int reset);

/* Experiment switches for the BVH8_CWBVH kernel of the next launches on this context (development aid; 0 = as shipped):
 * 1 = non-temporal ray loads / hit stores, 2 = the 64-byte triangle records in the ordinary kernels too (only where the scene has them:
 * after tbvh_cwbvh_set_hybrid or the first large launch; ignored otherwise) — both only in the experiment build (make EXPERIMENTS=1: the
 * shipped kernels do not carry the two code paths), 4 = a probed launch as ONE kernel even where the copies exist,
 * 8 = the next tbvh_cwbvh_set_hybrid / lazy build derives the node copy WITHOUT a triangle in each node's line, 16 = the coherent flavor of a two-flavor
 * launch takes the batch whatever its probe finds (tests put incoherent rays through the coherent schedules), 64 = no coherence probe (every
 * launch takes the unprobed path), bits 8..15 = waves per CU of the incoherent flavor (clamped to the 32 per CU the stack spill area is sized for). */
int tbvh_debug_set_flags(tbvh_context* ctx, uint32_t flags);

/* Which schedule the library has settled on for COHERENT batches of 2 M rays and more on this BVH8_CWBVH scene (closest-hit: anyhit = 0,
 * any-hit: 1) — the deferred-triangles + gated schedule on a third more waves, or the strict one.  No static property of a blob tells which
 * is faster (profiles/r04_sensitivity.txt: +1 ... +8 % for the first on most scenes, +10 % for the second on large-occluder scenes), so the
 * first few such launches alternate and are timed on the device (no synchronisation), then the faster stays (TBVH_COHERENT_TUNER=0 / 2 in
 * the environment pins the first / the second, 3 one traversal per wave).  out[0] = 0 still measuring, 1 deferred + gated, 2 strict, 3 one traversal per wave (kernels_cwbvh_packet.hip); out[1], out[2] = coherent samples
 * taken of each; out[3] = 1000 x best time per ray of the strict schedule / of the deferred one (0 until both have samples).  The choice is kept
 * per batch-size class (below 6 M rays, below 12 M, more: the end of a launch weighs differently — the atrium generator's camera rays are 15 % faster
 * strict at 16.7 M rays and even at 4.2 M); the call reports the class of the most recent launch. */
int tbvh_debug_coherent_schedule(tbvh_scene* scene, int anyhit, uint32_t out[4]);

/* The per-launch coherence probe of the most recent query on this context (development aid; DESIGN.md par. 3): out[0] = sampled
 * neighbouring ray pairs whose directions agree (and, for rays of finite reach, whose origins lie within 5 % of that reach), out[1] = pairs sampled, out[2] = 0 no probe ran (small batches, small or very
 * large scenes, other layouts), 1 the batch was classified incoherent (strict schedule), 2 coherent (deferred triangles, gated
 * triangle phase, a third more waves).  Synchronizes the stream. */
int tbvh_debug_last_probe(tbvh_context* ctx, uint32_t out[3]);

/* The two launch lanes of a context (tbvh_context_set_overlap): out[0] = query launches that went to the second lane since the context was made,
 * out[1] = joins taken (the first lane made to wait for the second one's last launch: by a launch that conflicted with launches on both lanes or found
 * its lane's list full, by a launch a schedule tuner measured, or by any other call on the context while the second lane held work). */
int tbvh_debug_overlap_stats(tbvh_context* ctx, uint64_t out[2]);
/* The rule that picks a launch's lane (tinybvh_amd/csrc/overlap_lanes.h), run over a script on the host; no device, no context.  ops5: n_ops rows of 5 x u64
 * {operation, a, b, c, d}.  0 = a launch touching ray bytes [a, b) and flag bytes [c, d) (c == d: none): finished launches are pruned, the lane is chosen, the
 * launch is recorded under its row number; out[row] = lane + 2 if the lanes were joined first.  1 = the launch of row a has finished.  2 = the second lane
 * is available (a != 0) or not.  3 = out[row] = launches in flight on lane 0 + 256 x those on lane 1, after pruning.  Other rows leave out[row] = 0. */
int tbvh_debug_lane_script(const uint64_t* ops5, uint64_t n_ops, int32_t* out);

/* How many launches one lane may START ahead of the other (TBVH_OVERLAP_DEPTH in the environment; 1 or 2, default 1).  1: a launch waits for the start of
 * the other lane's latest launch.  2: for the start of the other lane's launch before its latest one, while that one is in flight — a caller alternating
 * two buffers (camera rays, bounce rays) gets the next camera launch into the tail of the bounce launch before the last.  Footprint conflicts keep their
 * order at either depth. */
int tbvh_debug_set_overlap_depth(tbvh_context* ctx, int depth);
/* The context's memory of the coherence probe's verdicts (TBVH_PROBE_MEMORY=0 in the environment: off).  On (default): a probed two-flavor launch on a
 * buffer (the same ray range, closest or any hit, scene) whose last two FINISHED launches were both classified incoherent leaves out the coherent flavor,
 * which would only have sampled the probe and left; the incoherent flavor takes the sample, so the memory keeps learning and one coherent batch brings the
 * two flavors back.  Which rays are traced, and what is written, never depends on it.  Setting it forgets what was learnt. */
int tbvh_debug_set_probe_memory(tbvh_context* ctx, int enabled);
/* out[0] = launches that left out the coherent flavor since the context was made, out[1] = verdicts read back from finished launches. */
int tbvh_debug_probe_memory_stats(tbvh_context* ctx, uint64_t out[2]);
/* tbvh_debug_lane_script with the start rule at `depth` and the verdict memory (tinybvh_amd/csrc/overlap_lanes.h: LaneBook::gate, probe_memory.h); no device,
 * no context.  ops6: n_ops rows of 6 x u64 {operation, a, b, c, d, e}; out2: two numbers per row, {0, -1} where nothing is said.  Operations 0 to 3 as in
 * tbvh_debug_lane_script (their answer in out2[2 row]); for a launch (0) out2[2 row + 1] = the row of the launch whose start it waits for, -1 for none.
 * 4 = a call that joins the lanes.  5 = a probed launch of ray bytes [a, b) on scene c, any hit if d != 0, on lane e: verdicts of finished launches are
 * harvested, out2[2 row] = 1 if it goes solo, and it is remembered under its row number.  6 = the probe of the launch of row a said b (1 incoherent,
 * 2 coherent, 0 nothing), read once that row is finished (operation 1). */
int tbvh_debug_runahead_script(const uint64_t* ops6, uint64_t n_ops, int depth, int64_t* out2);

/* What a query launch will do (tinybvh_amd/csrc/launch_plan.h: the functions launchQuery itself calls), from the facts it reads; no device, no context.
 * facts: n_facts = 22 words {is TLAS, layout, variant, blob bytes, rays, the host knows the size, any hit, grid override, CUs, persistent grid, rays per
 * block, debug flags, TBVH_COHERENT_TUNER's mode, the schedules settled for the four size classes, the scene has the padded node copy / the hybrid node copy /
 * the 64-byte triangle records, probe memory on, timing off}.  out: n_out = 15 words {small, huge, probed, probedSmall, probedSmall cancelled by a per-lane
 * schedule, size class, grid by size, grid of a coherent batch, 7-waves grid of the two-level kernels, of the BVH8_CWBVH kernels, a tuner may time it,
 * solo candidate, wants a verdict slot, shape of a BVH8_CWBVH launch (0 one kernel, 1 two flavors, 2 flavor + unprobed kernel behind, 3 / 4 / 5 variant
 * 90 / 91 / 92), padded node copy walked}.  TBVH_E_INVALID for other word counts or 0 rays per block. */
int tbvh_debug_launch_plan(const uint64_t* facts, uint32_t n_facts, uint32_t* out, uint32_t n_out);

/* Which two-level kernel serves a TLAS, and through which arrays it enters each BLAS (tinybvh_amd/csrc/tlas_plan.h: the function the library itself calls when
 * a TLAS is classified), from the facts it reads; no device, no context.  One case is 5 + n fact words {BLAS count n, the TLAS has had an any-hit query, its
 * nodes are on the device, nodes an 8-wide TLAS tree would need, blocks a 4-wide one would need} followed by one word per BLAS {layout | pinned by
 * tbvh_set_variant << 8 | has an 8-wide copy << 9 | has a 4-wide copy << 10}, and gives 13 + n plan words: for closest-hit queries {class layout (0 = mixed),
 * mix of BVH8_CWBVH and BVH_GPU, kernel family (0 flat loop with the sphere step, 1 k_tlas4, 2 k_tlas8, 3 voxel sets, 4 k_tlas2, 5 flat loop), bytes of a stack
 * entry}, the same four for any-hit queries, {any-hit queries have a class of their own, the 8-wide tree is wanted, it fits its index range, the 4-wide tree is
 * wanted, it fits} and one word per BLAS {closest-hit view | any-hit view << 8; 0 its own arrays, 1 its 8-wide copy, 2 its 4-wide copy}.  facts may hold
 * several cases back to back (n_words in all); out takes their plans back to back (n_out in all).  TBVH_E_INVALID when the word counts do not match. */
int tbvh_debug_tlas_plan(const uint64_t* facts, uint32_t n_words, uint32_t* out, uint32_t n_out);
/* The facts a live TLAS would state right now (facts_out: 5 + its BLAS count words) and the plan it has stored (plan_out: 13 + its BLAS count words), in the
 * words of tbvh_debug_tlas_plan.  The stored plan is the one its launches read: it equals the plan of the facts at all times.  Changes nothing, does not
 * synchronize.  TBVH_E_INVALID for a scene that is not a TLAS (or a BVH_DOUBLE one). */
int tbvh_debug_tlas_state(tbvh_scene* scene, uint64_t* facts_out, uint32_t* plan_out);

/* The wave-packet kernel's child filter (tinybvh_amd/csrc/packet_cull.h) beside its exact per-lane test, for ONE 64-ray chunk against n_nodes BVH8_CWBVH nodes
 * (80 bytes each), on the host as k_cwbvh_packet runs them; no device, no context.  rays64: 64 ray records of 64 bytes (O, D, rD, hit; O and rD are read);
 * have_mask: bit l = lane l holds a ray (at least one); tcull64: each lane's cull distance as the kernel forms it (cull_bound(hit.t), -1 for a ray that is out
 * of the game).  Per node: maybe_out = the children the wave's interval test lets through (every non-empty child where the filter is off), exact_out = the
 * children some lane's ray enters by the exact test.  exact is a subset of maybe, always; neither has a bit in an empty slot.  chunk_flags (may be NULL):
 * bit 0 = the lanes differ in octant, bit 1 = a ray with a non-finite origin or reciprocal direction — either turns the filter off for the chunk. */
int tbvh_debug_packet_cull(const void* nodes80, uint64_t n_nodes, const void* rays64, uint64_t have_mask, const float* tcull64, uint8_t* maybe_out,
                           uint8_t* exact_out, uint32_t* chunk_flags);

/* The ray / triangle test in its two forms (tinybvh_amd/csrc/device_common.h), on the host; no device, no context: tri_test with its early-outs (the per-lane
 * kernels) and tri_test_flat, the branch-free form of the wave-packet kernel.  n pairs: od6 = {O.xyz, D.xyz}, tri9 = {v0, e1 = v1 - v0, e2 = v2 - v0}, tmax = the
 * ray's closest hit so far (inclusive).  Per pair: accept_* = 1 when the form reports a hit, tuv_* = its {t, u, v} (the branching form writes them only when it
 * accepts: zeros otherwise; the flat form always).  The two must agree on accept, and bit for bit on t, u, v wherever they accept. */
int tbvh_debug_tri_test_flat(const float* od6, const float* tri9, const float* tmax, uint64_t n, uint8_t* accept_branch, uint8_t* accept_flat, float* tuv_branch,
                             float* tuv_flat);

/* tbvh_host_tri_test over n pairs (tests/test_watertight_host.py): rays64 = n ray records, tris9 = n x {v0, v1, v2}; accept: n bytes; tuv: n x 3 floats (0 where
 * rejected); uvw: NULL or n x 3 floats, the watertight test's edge functions U, V, W (test 1 only); roles: 0 = IntersectTri's vertex roles, 1 = TriOccludes'. */
int tbvh_debug_tri_test_batch(int test, int roles, const void* rays64, const float* tris9, uint64_t n, uint8_t* accept, float* tuv, float* uvw);

/* Diagnostic kernel variants of BVH8_CWBVH scenes (0 = default): 72 / 52 force the strict / the coherent schedule whatever
 * the probe says, 90 the incoherent flavor on the copies of tbvh_cwbvh_set_hybrid, 75 / 88 split the last rays whatever the batch size, 59 / 61 / 73 / 78 / 82 / 83 are the instrumented
 * kernels behind tbvh_debug_stats.  Returns TBVH_E_INVALID for anything else. */
int tbvh_set_variant(tbvh_scene* scene, int variant);

/* The BVH2 (tinybvh::BVH::BVHNode layout, 32 bytes per node, leaves of at most max_leaf_tris entries) the library derives on the HOST from an uploaded
 * BVH_GPU blob (layout 5: nodes64 + prim_idx + verts16) or BVH4_GPU stream (layout 8: blocks16 in `blob`, n_blob 16-byte blocks; prim_idx / verts16 unused)
 * before it collapses it into the scene's 8-wide copy (tinybvh_amd/csrc/capi_scene.hip: makeCopy).  No device involved: the tests walk the result
 * with the oracle.  Layout 5 with prim_idx == NULL = RECORD MODE, the form the library runs (the blob is read back from the device, where the triangles
 * live as gathered records): verts16 then holds n_idx records {v0|prim, e1 = v1 - v0, e2 = v2 - v0} of 48 bytes.  nodes32_out: cap_nodes x 32 bytes; recs_out (layout 8 only): the stream's triangle records {v0|prim, e1, e2} in the order the leaves
 * index them, cap_recs x 48 bytes.  Counts are returned also when a capacity is too small (TBVH_E_INVALID then): call twice.  TBVH_E_FORMAT: the root is
 * a leaf / the stream is malformed (no copy is made for such a blob). */
int tbvh_debug_wide_copy_bvh2(int layout, const void* blob, uint64_t n_blob, const uint32_t* prim_idx, uint64_t n_idx, const void* verts16, uint64_t n_tris,
                              uint32_t max_leaf_tris, void* nodes32_out, uint64_t cap_nodes, uint64_t* n_nodes_out, void* recs_out, uint64_t cap_recs,
                              uint64_t* n_recs_out);

/* The device SAH builder (tbvh_build_bvh2_sah_device, tbvh_build_device_sah) finishes subtrees of at most n primitives by one wave each, out of LDS,
 * instead of by its per-level kernels.  n = 0: the per-level path alone; n >= the triangle count: one wave builds the whole tree.  The tree does not
 * depend on n (tests force both paths); the build time does.  A new context starts at 64 (profiles/sah_device_build.txt). */
int tbvh_debug_set_sah_small_subtree(tbvh_context* ctx, uint32_t n);
/* Inputs of at most n primitives (triangles, boxes, spheres) are built by ONE workgroup in one launch (kernels_sahbuild.hip: k_sah_one_group: the level loop
 * with workgroup barriers in place of kernel boundaries, no read-back per level) instead of by the per-level kernels.  0: never.  Inputs of more than 2^14
 * primitives take the level path whatever n says.  The tree does not depend on n (tests force both paths); the build time does
 * (a new context starts at 3000: profiles/box_sah_build.txt has the sweep it was chosen from). */
int tbvh_debug_set_sah_one_group(tbvh_context* ctx, uint32_t n);
/* out[0] = the context's small-subtree threshold, out[1] = its one-workgroup threshold, as they are now (a test saves them before it changes them). */
int tbvh_debug_get_sah_thresholds(tbvh_context* ctx, uint32_t out[2]);

/* Device memory the library itself owns right now, over every context of this process: out[0] = live allocations, out[1] = their bytes.  Scenes (their
 * derived copies, staging and scratch areas included), contexts and wavefront objects are counted; memory handed to the caller (tbvh_device_malloc,
 * tbvh_pinned_malloc) and the library's pinned host buffers are not.  Both return to their earlier values once everything created since was freed:
 * what tests/test_device_memory.py asserts.  Needs no device and no context. */
int tbvh_debug_device_allocations(uint64_t out[2]);
/* tbvh_scene_device_bytes of any scene term by term, filled by the same list of terms (tinybvh_amd/csrc/capi_scene.hip: sceneBytesByWord): out[0] the arrays
 * as uploaded, converted or built, [1] the re-layouts of a BVH8_CWBVH scene (padded nodes, hybrid nodes, 64-byte triangle records), [2] the wide copies (each
 * copy's own tbvh_scene_device_bytes, now), [3] opacity maps (on the scene they were set on), [4] the index buffer a scene made from an indexed mesh holds,
 * [5] an fp32 TLAS's wide trees, references and SAH Wald nodes, or an fp64 TLAS's one allocation, [6] counted scratch and staging (sphere and fp64 scenes, the
 * SAH TLAS builder), [7] what the scene holds and does NOT count (a triangle scene's refit scratch and staging, the hybrid copy's numbering, a TLAS's shared
 * scratch, bounds, staged transforms and descriptor tables), at allocation size.  out[0] + ... + out[6] == tbvh_scene_device_bytes( scene ), always. */
int tbvh_debug_scene_bytes(const tbvh_scene* scene, uint64_t out[8]);

/* The core the device LBVH builders share (tinybvh_amd/csrc/lbvh.h), run on the host; no device, no context (tests/test_lbvh_host.py).
 * topology: the Karras range search over n sorted keys (key_bits 32: the low words are the keys; 64), for the interior nodes i = 0 .. n - 2:
 * out4[4 i ..] = {left, right, lo, hi}, the children in Karras ids (interior node g -> g, leaf g -> n - 1 + g) and the node's sorted range.  2 <= n < 2^31.
 * ordered: the order-preserving encoding of the centre bounds: bits 32: encoded[i] = the code of (float)values[i] and decoded[i] its decoding; 64: of values[i].
 * build_scratch_bytes: the scratch allocation of the six device builders for n primitives, given hipcub's temporary sizes: out = {LBVH, PLOC, fp32 TLAS,
 * fp64 TLAS, SAH, SBVH}. */
int tbvh_debug_lbvh_topology(const uint64_t* keys, uint64_t n, int key_bits, uint32_t* out4);
int tbvh_debug_lbvh_ordered(const double* values, uint64_t n, int bits, uint64_t* encoded, double* decoded);
int tbvh_debug_build_scratch_bytes(uint32_t n, uint64_t sort_temp_bytes, uint64_t scan_temp_bytes, uint64_t out[6]);

/* The device address of one of a scene graph's arrays (what: the TBVH_GRAPH_* codes of tbvh_scenegraph_download; TBVH_GRAPH_COMBINED: the last walk's), so that a
 * test can overwrite a table or a key state on the device and see the kernels' own range checks answer (tests/test_scenegraph_gpu.py).  Not for products: the
 * arrays are the graph's private state. */
struct tbvh_scenegraph;
int tbvh_debug_scenegraph_array(struct tbvh_scenegraph* g, int what, void** d_ptr);
/* ONE kernel of an advance as a timed operation of its own (tbvh_time_last_ms), for tools/scenegraph_anim_bench.py: step 0 = k_graph_sample over every channel
 * with dt, 1 = k_graph_local, 2 = k_graph_combine, 3 = k_graph_outputs.  Steps 0, 1, 2, 3 in this order are one tbvh_scenegraph_advance. */
int tbvh_debug_scenegraph_step(struct tbvh_scenegraph* g, int step, float dt);
/* Every node's T, R, S of a host graph replaced at once (n_nodes x 10 floats: translation, rotation w x y z, scale; n_nodes must be the graph's).  Which nodes
 * rebuild their local transform in the next walk stays as the channels left it.  For tests that pin the walk to given inputs. */
struct tbvh_host_scenegraph;
int tbvh_debug_host_scenegraph_set_trs(struct tbvh_host_scenegraph* g, const float* trs10, uint64_t n_nodes);
/* The host twin walks parent-first; the kernels multiply every node down its own ancestor list (k_graph_combine).  This runs THAT form on the CPU over the host
 * graph's lists, as the kernel does, and reports how many nodes' combined transforms differ in any bit from the last walk's (0 is the only right answer), so that
 * the lists sg_compile builds and their range checks are exercised without a GPU (tools/scenegraph_sanitize.cpp, tests/test_scenegraph_host.py). */
int tbvh_debug_host_scenegraph_check_chains(struct tbvh_host_scenegraph* g, uint64_t* n_differ);

/* The queues of a wavefront object as they stand after its last tbvh_wavefront_render, copied to the host so that a test can hold every path vertex to a
 * restatement (tests/test_wavefront_paths_gpu.py).  Not for products: the queues are the path tracer's private state.  Every buffer takes width x height
 * records (the capacity; the counters say how many are live) and may be NULL: rays0 / rays1 the two path queues (64-byte ray records), aux0 / aux1 their
 * PathAux (16 bytes: throughput, pixel << 8 | depth << 4 | flags), shadow / shadow_aux the shadow queue (16 bytes: contribution, pixel), occ its any-hit
 * flags (one byte each).  counters[d] = entries of the path queue depth d read (d = 0 .. 8), counters[9 + d] = entries of the shadow queue depth d filled.
 * After a render with max_depth K: rays[(K - 1) & 1] is the input of the last Shade with Extend's hit records; for K >= 2 rays[(K - 2) & 1] is the input of
 * the Shade before it (the last stage writes no bounce rays); the shadow queue and occ are stage K - 1's.  Synchronizes the stream, changes nothing on the
 * device.  Call it BEFORE tbvh_wavefront_finalize: that reuses the shadow-ray buffer for its pixels. */
int tbvh_debug_wavefront_queues(tbvh_wavefront* w, void* rays0, void* aux0, void* rays1, void* aux1, void* shadow, void* shadow_aux, uint8_t* occ,
                                uint64_t counters[18]);

/* viewer.h's own atan2f (kind 0: out[i] = atan2( a[i], b[i] )) and acosf (kind 1: out[i] = acos( a[i] ), b not read) on the CPU, for tools/viewer_math_error.c,
 * which measures their distance from float64 libm (DESIGN.md par. 22: the SKY_EDGE margin).  Host arrays, no context. */
int tbvh_debug_viewer_math(int kind, const float* a, const float* b, uint64_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif /* TINYBVH_AMD_DEBUG_H_ */

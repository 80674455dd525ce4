/* gnr.h -- C ABI of the MI355X-native GraspNeRF volumetric hot path (libgnr.so).
 *
 * Drop-in boundary for the reference's `NeuralRayRenderer.sample_volume` / `.render`
 * (ref: src/nr/network/renderer.py:164-199, :201-220, :110-138) for a BATCH of scenes.
 * Plain pointers and sizes only: every `const float*` below is a DEVICE pointer to
 * contiguous fp32 unless the name says `_host`.  `stream` is a hipStream_t passed as void*.
 * All entry points are stateless and return 0 (GNR_OK) or a negative error code; nothing
 * throws across the ABI.  The caller owns every buffer, including the workspace.  STATELESS is
 * meant literally: the library keeps no mutable switch -- what a call computes depends on its arguments alone (the per-call
 * switches are GnrScene.options / the `options` argument of the entry points without a scene), so two callers, or two streams,
 * of one process can hold different settings.  (The only process-wide state is the opt-in measurement tooling at the end of
 * this header, which adds event brackets around launches and changes nothing they compute.)
 *
 * Typical call sequence (what graspnerf_amd/renderer.py does through ctypes):
 *   gnr_pack_weights(canonical_host, packed_host)         once per load_state_dict, per level
 *   gnr_workspace_bytes(&scene, R, rn, dn)                once per shape
 *   gnr_prepare(&scene, ws, ws_bytes, stream)             per forward (feature-map repack)
 *   gnr_sample_volume_fwd(...) / gnr_render_rays_fwd(...) per forward
 */
#ifndef GNR_H
#define GNR_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNR_OK 0
#define GNR_ERR_ARG (-1)       /* null pointer / bad enum                                   */
#define GNR_ERR_SHAPE (-2)     /* unsupported V, dn, feature width ...                      */
#define GNR_ERR_HIP (-3)       /* a HIP call or kernel launch failed                        */
#define GNR_ERR_WORKSPACE (-4) /* workspace too small                                       */
/* One error text per thread for the whole library: after a call that returned an error, gnr_last_error() names the refusal, or
 * the kernel launch / HIP call that failed and hipGetErrorString of its error ("<label or call>: <text>").  gnr_head_last_error,
 * gnr_post_last_error, gnr_img_last_error and gnr_ingest_last_error are aliases of it, kept for existing callers: all five return
 * the text of the thread's last failed call, whichever source file its entry point lives in. */

/* Reference views of B scenes.  Replaces the `ref_imgs_info` dict
 * (ref: src/nr/utils/imgs_info.py:120, src/nr/main.py:228-242) after the 2D backbones
 * (renderer.py:275-279) have produced img_feats / ray_feats. */
typedef struct GnrScene {
    int B, V;                 /* scenes, views per scene (V in 2..8)                        */
    int H, W;                 /* image size                                                 */
    int fh, fw;               /* feature-map size (reference: H/4, W/4)                     */
    const float* imgs;        /* [B,V,3,H,W]  in [0,1]                                      */
    const float* img_feats;   /* [B,V,32,fh,fw]  image_encoder output   (renderer.py:275)   */
    const float* ray_feats;   /* [B,V,32,fh,fw]  vis_encoder output     (renderer.py:279)   */
    const float* poses;       /* [B,V,3,4] world->camera, OpenCV                            */
    const float* Ks;          /* [B,V,3,3]                                                  */
    const float* depth_range; /* [B,V,2] near, far                                          */
    int use_vis;              /* cfg dist_decoder_cfg.use_vis (both levels, dist_decoder.py:89-97): 1 -> the packed level
                                 blobs were completed with gnr_pack_vis_decoder (training: the backward blobs with
                                 gnr_pack_vis_decoder_bwd) and the chain runs the fourth decoder branch; the gradient
                                 blobs of the *_bwd entry points then have gnr_canonical_weights_floats() +
                                 gnr_canonical_vis_floats() floats; 0 -> configs/nrvgn_sdf.yaml                          */
    unsigned options;         /* per-call switches, an OR of GNR_OPT_* below; 0 = the product path.  Unknown bits: GNR_ERR_ARG   */
} GnrScene;

/* ---- per-call options (GnrScene.options; `options` of gnr_ray_tail_dual_bwd / gnr_geo_dual_bwd) -------------
 * Product switches:
 *   GNR_OPT_FEATURE_GRAD_FIXED  the feature-map gradients of this call (gnr_depth_mean_bwd, gnr_sample_volume_bwd,
 *                               gnr_render_chain_bwd) are BIT-REPRODUCIBLE: 64-bit fixed-point adds instead of float sums in
 *                               arrival order (see "backward twins" below).  Since round 6 the view kernels' binned scatter sums
 *                               the same parked rows as integers: the mode costs what the float mode costs.
 * Measurement / test switches (same results to rounding unless stated):
 *   GNR_OPT_FP32_CHAIN          every chain launch of the call -- forward, training forward and the backward's view kernels -- runs
 *                               its fp32-input-MFMA instantiation (what the range guard falls back to); the pair kernels are skipped
 *   GNR_OPT_VIEW1_ONE_WAVEFRONT / GNR_OPT_VIEW2_ONE_WAVEFRONT   the backward of the first / second view loop as one wavefront per tile
 *                               (k_view1_bwd / k_view2_bwd) instead of a compute wavefront and its partner (k_view*_bwd_pw)
 *   GNR_OPT_DIRECT_SCATTER      the feature-map gradient of k_view1_bwd_pw as direct float atomics instead of the binned scatter
 *                               (csrc/gnr_bwd_scatter.inc: rows parked in HBM, summed per feature-map pixel first)
 *   GNR_OPT_RAY_ORDER_MORTON    the inference render passes traverse a scene's rays in the Morton order of their pixels (internal
 *                               layout only; every array of the ABI keeps the caller's ray order, results are bit-identical)
 *   GNR_OPT_GEO_DUAL_FP32       gnr_geo_dual_fwd and the per-point half of gnr_geo_dual_bwd as fp32 FMAs, one lane per point, instead of the fp16-pair chain
 *   GNR_OPT_POISON_PARTIALS     the partial-gradient buffers are filled with NaN patterns before the kernels run (an entry no wavefront
 *                               stores would show in the reduced gradient)
 *   GNR_OPT_STATIC_TILES        the chain launches of the call give every wavefront its static round-robin share of the tiles instead of
 *                               handing the tiles out through the workspace's per-XCD counters (round 6; bit-identical outputs, the
 *                               launches' tails are longer: tests, measurements)
 *   GNR_OPT_SPLIT_LAUNCH        (experiment) gnr_sample_volume_fwd runs the two halves of the batch as two launch sequences on two streams (the
 *                               caller's and a library-owned one, joined before the call returns its stream), so that each half's
 *                               launches fill the other's tails; bit-identical outputs
 *   GNR_OPT_SAMPLE_ORDER_NATURAL  the inference render passes keep the natural (ray, sample) order of their points instead of the view-mask order
 *                               (see "sample order" below; bit-identical outputs: tests, A/B measurements)
 *   GNR_OPT_TEST_LOSE_PARTNER   (tests) the partner wavefronts of k_view1_bwd_pw / k_view2_bwd_pw return at once: the compute wavefronts'
 *                               bounded waits give up, the call's gradients are garbage and bit 4 of gnr_range_status says so */
#define GNR_OPT_FP32_CHAIN 0x001u
#define GNR_OPT_FEATURE_GRAD_FIXED 0x002u
#define GNR_OPT_VIEW1_ONE_WAVEFRONT 0x004u
#define GNR_OPT_VIEW2_ONE_WAVEFRONT 0x008u
#define GNR_OPT_RAY_ORDER_MORTON 0x010u
#define GNR_OPT_POISON_PARTIALS 0x020u
#define GNR_OPT_DIRECT_SCATTER 0x040u
#define GNR_OPT_GEO_DUAL_FP32 0x080u
#define GNR_OPT_TEST_LOSE_PARTNER 0x100u
#define GNR_OPT_STATIC_TILES 0x200u
#define GNR_OPT_SPLIT_LAUNCH 0x400u
#define GNR_OPT_SAMPLE_ORDER_NATURAL 0x800u
#define GNR_OPT_ALL 0xfffu

/* Query rays of B scenes.  Replaces the `que_imgs_info` dict (imgs_info.py:126-135). */
typedef struct GnrRays {
    int rn;                   /* rays per scene                                             */
    int dn;                   /* coarse samples per ray   (cfg depth_sample_num)            */
    int fdn;                  /* fine samples per ray     (cfg fine_depth_sample_num)       */
    int ray_mask_view_num;    /* cfg ray_mask_view_num  (renderer.py:37)                    */
    int ray_mask_point_num;   /* cfg ray_mask_point_num (renderer.py:38)                    */
    const float* coords;      /* [B,rn,2] pixel (x,y)                                       */
    const float* que_pose;    /* [B,3,4]                                                    */
    const float* que_K;       /* [B,3,3]                                                    */
    const float* que_depth_range; /* [B,2]                                                  */
    const float* que_imgs;    /* [B,3,H,W] or NULL (then pixel_colors_gt is not written)    */
    const float* fine_u;      /* [B,rn,fdn] in [0,1) or NULL.  is_train=True draws the inverse-CDF
                                 samples with torch.rand (render_ops.py:204-205): the caller draws them
                                 (same generator, same shape as the reference) and passes them here;
                                 NULL = eval mode, u_i = (i+.5)/fdn (render_ops.py:200-203)            */
    int ray_batch_num;        /* cfg ray_batch_num (renderer.py:203-215): the reference renders rays in
                                 chunks and returns one sdf_gradient_error per chunk; >0 -> the output
                                 is [B, ceil(rn/ray_batch_num)] chunk means, 0 -> one mean per scene   */
    int fine_depth_use_all;   /* cfg fine_depth_use_all (renderer.py:145-146): 1 -> the fine pass renders the dn coarse and
                                 the fdn resampled depths of a ray, merged and sorted (dn + fdn <= 128 samples; the fine level's
                                 positional table must have been built for that length, i.e. fine_agg_net_cfg.sample_num =
                                 dn + fdn in the reference); 0 -> the fdn resampled depths only                              */
} GnrRays;

/* Outputs of one render pass (coarse or fine).  Keys follow renderer.py:90-138; any
 * pointer may be NULL to skip that output.  `dn` below = GnrRays.dn (coarse) / .fdn (fine). */
typedef struct GnrRenderOut {
    float* depth;              /* [B,rn,dn] sample depths used by this pass                 */
    float* sdf_values;         /* [B,rn,dn]                                                 */
    float* alpha_values;       /* [B,rn,dn]                                                 */
    float* colors_nr;          /* [B,rn,dn,3]  (required: also an internal hand-off)        */
    float* hit_prob_nr;        /* [B,rn,dn]                                                 */
    float* pixel_colors_nr;    /* [B,rn,3]                                                  */
    float* pixel_colors_gt;    /* [B,rn,3]                                                  */
    float* render_depth;       /* [B,rn]                                                    */
    unsigned char* ray_mask;   /* [B,rn] 0/1                                                */
    float* sdf_gradient_error; /* [B, n_chunks] mean((|grad|-1)^2) per chunk of ray_batch_num rays
                                  (n_chunks = 1 when GnrRays.ray_batch_num == 0)            */
    float* sdf_gradient;       /* [B,rn,dn,3] optional (debug / eikonal loss)               */
    unsigned char* view_mask;  /* [B,rn,dn] optional: bit v = point inside view v's image   */
} GnrRenderOut;

/* ---- weights ---------------------------------------------------------------------------
 * canonical blob = the parameters of ONE level (decoder + aggregation net) flattened and
 * concatenated in reference state-dict order:
 *   <dec>.mean_decoder.{0,2,4}.{weight,bias}, <dec>.var_decoder..., <dec>.aw_decoder...,
 *   <agg>.prob_embed.{0,2}, <agg>.agg_impl.{ray_dir_fc,base_fc,vis_fc,vis_fc2,geometry_fc}.{0,2},
 *   <agg>.agg_impl.ray_attention.{w_qs,w_ks,w_vs,fc}.weight, .layer_norm.{weight,bias},
 *   <agg>.agg_impl.out_geometry_fc.{0,1}, .rgb_fc.{0,2,4}, .neuray_fc.{0,2},
 *   <agg>.deviation_network.variance
 * with <dec>,<agg> = dist_decoder,agg_net (coarse) or fine_dist_decoder,fine_agg_net (fine).
 * (ref: dist_decoder.py:64-88, aggregate_net.py:29-33, ibrnet.py:382-423, neus.py:9)      */
int gnr_canonical_weights_floats(void);   /* 36958 */
int gnr_packed_weights_floats(void);
/* Host-side packer: MFMA fragments of every layer (fp32), the tables of the per-ray kernel, and the image the chain kernel
 * stages into LDS, in which the wide layers' weights are stored as fp16 pairs w = h + m 2^-11 (1 fp32 ulp; csrc/gnr_layout.h
 * section C16).  GNR_ERR_ARG if a pointer is null.  An effective weight outside the fp16 range (|w| >= 65520) has no pair: the
 * blob is marked and every chain launch with it runs on the fp32-input MFMA (gnr_range_status bit 2). */
int gnr_pack_weights(const float* canonical_host, float* packed_host);
/* Optional: the fourth decoder branch of a level (cfg dist_decoder_cfg.use_vis: true; dist_decoder.py:89-97,103-104,133-134:
 * its sigmoid output multiplies both cdfs) into a blob gnr_pack_weights has filled.  vis_decoder_host = vis_decoder.{0.weight
 * [32][32], 0.bias [32], 2.weight [32][32], 2.bias [32], 4.weight [1][32], 4.bias [1]} in state-dict order (2145 floats).
 * Training (GnrScene.use_vis = 1 in gnr_sample_volume_fwd_train / _bwd, gnr_render_chain_fwd_train / _bwd): the same six tensors
 * go into the backward blob with gnr_pack_vis_decoder_bwd (after gnr_pack_weights_bwd), and the gradient blob `d_canonical`
 * carries their gradients BEHIND the level's 36958 floats, in the same state-dict order: gnr_canonical_vis_floats() = 2145
 * more.  (gnr_depth_mean_* reads mean_decoder only and takes no notice.) */
int gnr_pack_vis_decoder(const float* vis_decoder_host, float* packed_host);
int gnr_pack_vis_decoder_bwd(const float* vis_decoder_host, float* packed_bwd_host);
int gnr_canonical_vis_floats(void);       /* 2145 */
/* Device-side packers (csrc/gnr_pack_dev.hip): the same blobs from canonical blobs that are ALREADY ON THE DEVICE -- the training
 * loop's parameters move every optimiser step and, as in the reference (train/trainer.py:146-158: nn.Module parameters, optimiser
 * step on the device), never visit the host: no device-to-host copy, no host pack, no upload, no wait.  Stream-ordered kernels,
 * nothing synchronises.  The arithmetic is the host packer's own source (csrc/gnr_pack_body.h) and the results are bit-identical
 * to it.  The blobs are re-packed IN PLACE: `packed_dev` / `packed_bwd_dev` must once have been filled from a blob of
 * gnr_pack_weights / gnr_pack_weights_bwd (any weights) -- the constant parts (structural zeros, the position table) are kept.
 * gnr_pack_vis_decoder_device / _bwd_device: the use_vis branch, after the level's own re-pack, as on the host. */
int gnr_pack_weights_device(const float* canonical_dev, float* packed_dev, void* stream);
int gnr_pack_weights_bwd_device(const float* canonical_dev, float* packed_bwd_dev, void* stream);
int gnr_pack_vis_decoder_device(const float* vis_decoder_dev, float* packed_dev, void* stream);
int gnr_pack_vis_decoder_bwd_device(const float* vis_decoder_dev, float* packed_bwd_dev, void* stream);
/* float offset of a named section of the packed blob (see csrc/gnr_layout.h), -1 if unknown */
int gnr_layout_offset(const char* name);

/* ---- workspace -------------------------------------------------------------------------*/
size_t gnr_workspace_bytes(const GnrScene* scene, int volume_res, int rn, int dn_max);

/* Repack img_feats/ray_feats to channel-last and build the per-view projection blocks.
 * Must precede the forward calls that use the same workspace (stream ordered). */
int gnr_prepare(const GnrScene* scene, void* workspace, size_t workspace_bytes, void* stream);

/* Range guard.  The reference computes in fp32 everywhere (ibrnet.py:474-482; SURVEY.md 5 "mixed precision: none").  The chain
 * kernel multiplies on the f16 matrix cores with every fp32 operand carried as an fp16 pair, whose high half cannot hold a
 * magnitude of 65 520 or more.  Each forward (and training-forward) chain launch therefore watches its operands (feature maps in
 * gnr_prepare, activations and cross-view statistics in the kernel) and is followed by its fp32-input-MFMA twin, which returns
 * immediately unless the watch tripped and otherwise recomputes the launch: out-of-range scenes get the fp32 kernel's values,
 * in-range scenes pay ~5 us per chain launch, and no call synchronises with the host.
 * gnr_range_status reads the status words of the last gnr_prepare on this workspace (synchronises `stream`):
 *   bit 0: a feature-map value >= 6e4 in magnitude or not finite;  bit 1: an activation / statistic beyond the fp16 range (k_chain), or a
 *   non-finite value in the matrix-core tail of the per-ray kernel (an operand or a per-ray weight beyond the fp16 range: that launch and the
 *   later per-ray launches on the prepared scene are recomputed by their fp32 instantiation);
 *   bit 2: a weight beyond the fp16 range (gnr_pack_weights marks such a blob instead of refusing it);
 *   bit 3: (backward, GNR_OPT_FEATURE_GRAD_FIXED only) a feature-map gradient contribution was clamped to the fixed-point range;
 *   bit 4: (backward) GNR_STATUS_LOST_PARTNER -- a wavefront of k_view1_bwd_pw / k_view2_bwd_pw waited ~2^22 polls for its partner and
 *          gave up: THE GRADIENTS OF THAT BACKWARD CALL ARE INVALID.  The entry points still return GNR_OK (nothing synchronises with the
 *          host); a training loop must not apply such a step (graspnerf_amd/trainer.py skips the optimiser step on the device).
 * Bits 0 and 2 hold for every launch on the prepared scene (the pair kernel then returns at once and the twin computes the launch);
 * bit 1 is watched per launch slot (volume, coarse pass, fine pass, the training forwards), so a scene whose coarse pass tripped it
 * does not pay the recomputation on its volume or fine pass; the status word is the OR over the slots.
 * The backward twins follow the same guard (round 6): gnr_sample_volume_bwd / gnr_render_chain_bwd launch their fp16-pair view kernels
 * and, behind each, the fp32-input-MFMA instantiation; the former return at once when bits 0 / 2 of the scene or bit 1 of the pass's
 * training forward are set, the latter unless -- a range-tripped pass gets bitwise the gradients of GNR_OPT_FP32_CHAIN.
 * gnr_status_words_offset: byte offset of the 64 status words (unsigned) inside the workspace, for callers that test them on the device
 * (OR of the words & GNR_STATUS_LOST_PARTNER) instead of synchronising. */
#define GNR_STATUS_LOST_PARTNER 16u
int gnr_range_status(const GnrScene* scene, const void* workspace, size_t workspace_bytes, unsigned* flags_out, void* stream);
size_t gnr_status_words_offset(const GnrScene* scene);

/* sample_volume (renderer.py:164-199), volume_type [sdf]:
 *   sdf_out[b,x,y,z] for voxel centre bbox_min[b] + ((x,y,z)+.5)*(0.3/res).
 *   view_mask_out: optional [B, res^3] bytes in (x,y,z) order, bit v = in-image mask of view v. */
int gnr_sample_volume_fwd(const GnrScene* scene, const float* bbox_min /*[B,3]*/, int volume_res,
                          const float* packed_coarse /*device*/, float* sdf_out /*[B,res,res,res]*/,
                          unsigned char* view_mask_out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* The SDF gradient volume: what the reference's network returns next to the SDF on every sample_volume call and its volume path drops
 * (ibrnet.py:485-513, aggregate_net.py:133-134).  The volume is evaluated as res^2 columns (x, y) of res samples, top -> down
 * (renderer.py:167-179), query direction (0,0,1);  grad_out[b,x,y,z,:] = sum over the samples i of voxel (x,y,z)'s column of
 * d sdf_i / d p_(x,y,z) -- the VJP with ones through embedder, geometry_fc, positional table, the column's attention, LayerNorm,
 * out_geometry_fc, clip and fill, with the cross-view statistics held constant: the SUMMED VJP of the reference, NOT the per-point
 * Jacobian diagonal.  Components are in the world frame.  The same arithmetic as GnrRenderOut.sdf_gradient of a render pass.
 *   volume_res     3..64 (the per-column kernel with the VJP takes 3 to 64 samples)
 *   grad_out       [B,res,res,res,3]
 *   sdf_out        optional [B,res,res,res]: the SDF of this pass (through the render-record chain; measured bitwise equal to the volume
 *                  entry point's on the 3-view 16^3 test scene, which is not a promise: callers take the volume from that entry point)
 *   grad_error_out optional [B]: mean((|grad| - 1)^2) over the scene's res^3 voxels (the eikonal term, aggregate_net.py:139)
 *   workspace      the prepared scene's, of at least the sizing function below (it exceeds the workspace of the other forwards for the same res)
 * Runs on a prepared scene like the other forwards, before or after them: neither changes the other's bits.  It re-uses the per-call part
 * of the workspace, so it must NOT run between a training forward and its backward.  Range guard: status slot 7 (the chain launch) and
 * 8 (the per-column kernel's matrix-core tail), tile counters of its own; a tripped watch makes the fp32 twins behind the launches
 * recompute them, as for the other slots.  Capture-safe: the caller's stream only, no allocation, no host wait. */
size_t gnr_sample_volume_grad_workspace_bytes(const GnrScene* scene, int volume_res);
int gnr_sample_volume_grad_fwd(const GnrScene* scene, const float* bbox_min /*[B,3]*/, int volume_res,
                               const float* packed_coarse /*device*/, float* grad_out /*[B,res,res,res,3]*/,
                               float* sdf_out /*optional [B,res,res,res]*/, float* grad_error_out /*optional [B]*/,
                               void* workspace, size_t workspace_bytes, void* stream);

/* render_by_depth (renderer.py:110-138): one pass over given sample depths [B,rn,dn]
 * (ascending along each ray).  `level_weights` = packed coarse or fine blob (device). */
int gnr_render_by_depth_fwd(const GnrScene* scene, const GnrRays* rays, const float* depth, int dn,
                            const float* level_weights, GnrRenderOut* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* render (renderer.py:140-162, :201-220), eval mode: coarse pass on disparity-uniform
 * depths, inverse-CDF fine resampling (render_ops.py:172-229) + sort, fine pass.
 *   fine_depth_in : optional [B,rn,fdn]; when given it replaces the resampled depths
 *   fine_inds_out : optional [B,rn,fdn] int32 searchsorted indices of the resampling
 *   fine == NULL  : cfg use_hierarchical_sampling false (renderer.py:153-162): the coarse pass only -- no resampling, no fine
 *                   pass, packed_fine is not read (fine_depth_in / fine_inds_out must be NULL)                                  */
int gnr_render_rays_fwd(const GnrScene* scene, const GnrRays* rays, const float* packed_coarse,
                        const float* packed_fine, GnrRenderOut* coarse, GnrRenderOut* fine,
                        const float* fine_depth_in, int* fine_inds_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Sample order of the inference render passes (gnr_render_by_depth_fwd, both passes of gnr_render_rays_fwd).  The chain kernel works on
 * tiles of 16 points and skips a view for a tile when all 16 points project outside it.  Before its chain launch a pass therefore computes
 * one key byte per sample (bit v = the sample lies inside view v) and a per-scene permutation that groups the samples by key (more views
 * first; the sorted 16-sample groups dealt round-robin into 8 stripes of the scene's tiles: csrc/gnr_sample_order.h), and slot n of scene b
 * processes point perm[b][n].  A point's results do not depend on its tile, so every output is bit-identical to the natural order's, and
 * every array of the ABI keeps the caller's layout.  The workspace holds 5 bytes per ray sample for it (reserved for every sample count,
 * so that gnr_workspace_bytes grows with rn * dn_max).
 * A pass keeps the natural order when
 *   - GNR_OPT_SAMPLE_ORDER_NATURAL is set;
 *   - a scene has more than 2^18 samples in the pass (every workgroup of the placement counts all the keys of its scene);
 *   - the chain launch has fewer than 8 tiles per wavefront slot of the device (B * ceil(rn*dn/16) < 8 * 8 * CUs = 16 384 on MI355X; at
 *     512 rays x 40 samples: fewer than 13 scenes).  A launch of a tile or two per slot lasts as long as its longest tiles in any order
 *     (B = 1: no gain at all).  The 8 is the break-even of the EARLIER sort (one workgroup per scene, 43 us per pass at any B: measured
 *     at B = 1, 2, 4, 8, 32 the step lost 0.05 ms at B = 4, 0.02 ms at B = 8 and won 0.10 ms at B = 32, profiles/sample_order_ab.json).
 *     The placement now runs one workgroup per 4096 samples (csrc/gnr_kernels.hip k_sample_order); its break-even has NOT been measured
 *     yet (profiles/sample_place_ab.json says what was and was not), so the threshold stays where the last measurement put it.
 * Test tooling: gnr_debug_render_by_depth_perm = gnr_render_by_depth_fwd with a caller-given sample_perm [B][rn*dn] (int32, device; every
 * row a permutation of 0 .. rn*dn-1; entries are clamped into the scene); gnr_debug_sample_order = the device sort alone, keys [B][P] ->
 * perm [B][P] (P <= 2^18; the kernel loads the keys as aligned 16-byte words: when `keys` or `keys + B * P` is not 16-byte aligned it READS,
 * and does not use, up to 15 bytes in front of / behind the array, inside the aligned word that holds the array's first / last byte and
 * so inside that byte's page); gnr_sample_order_host = the same permutation of one scene computed on the host (no device work);
 * gnr_sample_order_host_chunked = the same again, computed the way the kernel does: chunk by chunk, every chunk of `chunk` samples from
 * the scene's histogram, the histogram of the keys in front of the chunk and the rank inside the chunk (csrc/gnr_sample_order.h);
 * gnr_sample_order_offsets = byte offsets of the last pass's keys / permutation in a workspace carved for (rn, dn_max). */
int gnr_debug_render_by_depth_perm(const GnrScene* scene, const GnrRays* rays, const float* depth, int dn, const float* level_weights,
                                   GnrRenderOut* out, const int* sample_perm, void* workspace, size_t workspace_bytes, void* stream);
int gnr_debug_sample_order(const unsigned char* keys, int B, int P, int* perm, void* stream);
int gnr_sample_order_host(const unsigned char* keys_host, int P, int* perm_out_host);
int gnr_sample_order_host_chunked(const unsigned char* keys_host, int P, int chunk, int* perm_out_host);
int gnr_sample_order_offsets(const GnrScene* scene, int rn, int dn_max, size_t* keys_offset, size_t* perm_offset);

/* fine_depth_use_all under training (renderer.py:145-146: the fine pass renders torch.sort(torch.cat([coarse depths, resampled depths])))
 * -- depth_a [nrays,na], depth_b [nrays,nb], each ascending per ray -> out [nrays,na+nb] ascending (na + nb <= 128).  The inference
 * entry point gnr_render_rays_fwd does this merge itself (GnrRays.fine_depth_use_all). */
int gnr_merge_depths(const float* depth_a, int na, const float* depth_b, int nb, float* out, int nrays, void* stream);

/* predict_mean_for_depth_loss (renderer.py:222-266) for one level: bilinear gather of ray_feats at
 * `coords` [B,pn,2] (x,y in full-res pixels, shared by the V views of a scene; the caller keeps the
 * reference's (row,col)-as-(x,y) quirk) + the decoder mean branch.  mean_out [B,V,pn,2]. */
int gnr_depth_mean_fwd(const GnrScene* scene, const float* coords, int pn, const float* level_weights,
                       float* mean_out, void* workspace, size_t workspace_bytes, void* stream);

/* Bring-up aid: per-point intermediates of the chain kernel on the volume points (column order,
 * top->down); dbg is [B*res^3][32] floats, layout documented at the definition (gnr_capi.inc). */
int gnr_debug_volume_chain(const GnrScene* scene, const float* bbox_min, int volume_res,
                           const float* packed_coarse, float* dbg, void* workspace,
                           size_t workspace_bytes, void* stream);

/* ---- grasp head: gd.networks.ConvNet.forward (src/gd/networks.py:48-54) --------
 * canonical blob = ConvNet state dict flattened in order: encoder.conv{1,2,3}, decoder.conv{1,2,3}, conv_qual,
 * conv_rot, conv_width (each .weight [Cout,Cin,k,k,k] then .bias).  volume [B,1,R,R,R] -> qual [B,1,40,40,40],
 * rot [B,4,40,40,40] (unit quaternions), width [B,1,40,40,40]. */
int gnr_head_canonical_floats(void);
int gnr_head_packed_floats(void);
int gnr_pack_grasp_head(const float* canonical_host, float* packed_host);
size_t gnr_grasp_head_workspace_bytes(int B, int volume_res);
int gnr_grasp_head_fwd(int B, int volume_res, const float* volume, const float* packed_head, float* qual, float* rot,
                       float* width, void* workspace, size_t workspace_bytes, void* stream);
const char* gnr_head_last_error(void);       /* alias of gnr_last_error() */
/* Weight gradient of a stride-1, padding K/2 3D convolution (the grasp head under autograd; MIOpen spends 75 ms on the
 * fused 16 -> 6 k5 head at 40^3, batch 8): dw [Cout,Cin,K,K,K] is ACCUMULATED; x [B,Cin,D,H,W], dy [B,Cout,D,H,W]. */
int gnr_conv3d_bwd_weight(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int K,
                          void* stream);

/* Stride-1, same-padding (K/2) 3D convolution on fp32 MFMA for the grasp head under autograd (gd/networks.py:30-37,91-96: the
 * two k5 layers at 20^3 / 40^3), K = 3 or 5.  w = the layer's canonical weights [Cout][Cin][K][K][K] on the device; the MFMA
 * fragments are packed on the device into `workspace` (gnr_conv3d_same_workspace_bytes) at every call, the weights move
 * every optimiser step.
 *   mode 0 (forward):        x [B][Cin][D][H][W]       -> y  [B][Cout][D][H][W]  (+ bias [Cout], or NULL)
 *   mode 1 (backward data):  x = dy [B][Cout][D][H][W] -> y = dx [B][Cin][D][H][W]  (transposed, flipped weights; bias ignored) */
/*   gnr_conv3d_same_bwd_weight: dw [Cout][Cin][K][K][K] is ACCUMULATED from x [B][Cin][D][H][W] and dy [B][Cout][D][H][W]
 *   (LDS-staged successor of gnr_conv3d_bwd_weight for K = 3 / 5; the workgroups' partial blocks go through `workspace` and
 *   are summed by a second kernel instead of hundreds of workgroups adding atomically into the same few thousand weights). */
size_t gnr_conv3d_same_workspace_bytes(int Cin, int Cout, int K);
size_t gnr_conv3d_same_bwd_weight_workspace_bytes(int B, int Cin, int Cout, int D, int H, int W, int K);
int gnr_conv3d_same_bwd_weight(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int K,
                               void* workspace, size_t workspace_bytes, void* stream);
int gnr_conv3d_same(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int D, int H, int W, int K,
                    int mode, void* workspace, size_t workspace_bytes, void* stream);
/* Structurally sparse weights (round 4).  The encoder's stride-2 layers (gd/networks.py:33-37,59-76) run as ONE stride-1 k3 convolution
 * over the space-to-depth input (8 Cin channels, backbone.conv3d_stride2): of the 8 x 27 (parity, tap) slots per input channel 27 hold a
 * weight.  gnr_conv3d_tap_mask reads a pattern tensor [Cout][Cin][K^3] (non-zero = the weight exists; the STRUCTURE, not the values: a
 * weight that happens to be 0.0 still has a gradient) and writes gnr_conv3d_tap_mask_words(Cin, Cout) uint32 words: per (16 input
 * channels, 16 output channels) block the set of taps that exist.  The _masked entry points are gnr_conv3d_same /
 * gnr_conv3d_same_bwd_weight that skip the absent taps (mask == NULL: dense, the same as the plain entry points). */
#define GNR_CONV3D_FIRST_GEN 0x100   /* tests: OR into `mode` (gnr_conv3d_same*) / `K` (gnr_conv3d_same_bwd_weight*): the K = 3 call runs the
                                        first-generation kernels (the > 32 M voxel path) */
size_t gnr_conv3d_tap_mask_words(int Cin, int Cout);
int gnr_conv3d_tap_mask(const float* pattern, unsigned* mask, int Cin, int Cout, int K, void* stream);
int gnr_conv3d_same_masked(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int D, int H, int W,
                           int K, int mode, const unsigned* mask, void* workspace, size_t workspace_bytes, void* stream);
int gnr_conv3d_same_bwd_weight_masked(const float* x, const float* dy, float* dw, int B, int Cin, int Cout, int D, int H, int W, int K,
                                      const unsigned* mask, void* workspace, size_t workspace_bytes, void* stream);

/* ---- image-side streaming ops of the 2D feature extractors (csrc/gnr_img.hip) ----------------------------------
 * The residual U-Nets in front of the hot path (src/nr/network/ops.py:96-230, init_net.py:8-35, vis_encoder.py:6-22) are
 * convolutions (left to MIOpen) glued by instance norms, activations, reflect paddings and two bilinear upsamplings; these
 * entry points run the glue as single passes over the activation.  Layout: contiguous planes [planes = N*C][H][W] fp32.
 *
 * gnr_instnorm_act: y = act(InstanceNorm2d(x; weight, bias, eps) + res)   (ops.py:135-138: ELU; :101-121,215: ReLU, the
 *   block's identity as `res`; biased variance, eps inside the square root).  res may be NULL.  mean / rstd [planes] are
 *   written for the backward.  act: GNR_ACT_NONE / GNR_ACT_RELU / GNR_ACT_ELU (alpha = 1).
 * gnr_instnorm_act_bwd: with g = dy * act'(out):  dx = weight * rstd * (g - mean_hw(g) - xhat * mean_hw(g * xhat)),
 *   dres = g (NULL: not wanted), dbias[c] = sum_n sum_hw g, dweight[c] = sum_n sum_hw g * xhat (summed in a fixed order, no
 *   atomics; s1 / s2 [planes]: scratch for the per-plane sums).  `out` = the forward's y (may be NULL for GNR_ACT_NONE).
 * gnr_reflect_pad2d: F.pad(x, (pad,)*4, mode='reflect') as nn.Conv2d(padding_mode='reflect') applies it (ops.py:8,134,163):
 *   y [planes][H+2 pad][W+2 pad];  pad < min(H, W).  _bwd: dx[h][w] = sum of dy over the padded positions reading x[h][w].
 * gnr_upsample2x_bilinear: F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=True) (ops.py:147): y [planes][2H][2W].
 * All return GNR_OK / GNR_ERR_ARG (null pointer) / GNR_ERR_SHAPE / GNR_ERR_HIP; text in gnr_last_error(). */
#define GNR_ACT_NONE 0
#define GNR_ACT_RELU 1
#define GNR_ACT_ELU 2
const char* gnr_img_last_error(void);        /* alias of gnr_last_error() */
int gnr_instnorm_act(const float* x, const float* res, const float* weight, const float* bias, float* y, float* mean, float* rstd,
                     long long planes, int C, int HW, float eps, int act, void* stream);
int gnr_instnorm_act_bwd(const float* dy, const float* out, const float* x, const float* mean, const float* rstd, const float* weight,
                         float* dx, float* dres, float* s1, float* s2, float* dweight, float* dbias, long long planes, int C, int HW, int act,
                         void* stream);
int gnr_reflect_pad2d(const float* x, float* y, long long planes, int H, int W, int pad, void* stream);
int gnr_reflect_pad2d_bwd(const float* dy, float* dx, long long planes, int H, int W, int pad, void* stream);
int gnr_upsample2x_bilinear(const float* x, float* y, long long planes, int H, int W, void* stream);

/* ---- image ingest on the device (csrc/gnr_ingest.hip) -----------------------------------------------------------
 * The planner's image preparation (src/nr/main.py:167-172, 191-192: skimage imread(...)[:, :, :3] -> cv2.resize(img, wh),
 * INTER_LINEAR -> / 255 -> HWC to CHW) for n uint8 frames in ONE launch: out = float [n,3,dst_h,dst_w] in [0,1], bit-identical
 * to planner.resize_bilinear_u8(img, wh).astype(float32) / 255 transposed (OpenCV's fixed point: 11-bit coefficients,
 * (.. + 2) >> 2 in the vertical pass; the kernel is integer arithmetic plus a 256-entry table of float(i) / 255).
 * gnr_ingest_tables_host (host only, no device work) fills an opaque blob of gnr_ingest_tables_bytes(dst_h, dst_w) bytes with
 * the per-axis source indices and coefficients (float64 positions, no fused multiply-add) and that table; the caller uploads it
 * once per (src, dst) size and passes the device copy as tables_dev.
 * frames: DEVICE uint8, `channels` = 3 or 4 interleaved (a 4th channel is ignored), row y of frame f at
 * frames + f * frame_pitch + y * row_pitch (pitches in bytes).  Stream-ordered, no allocation, no host synchronisation.
 * GNR_ERR_ARG: null pointer, channels not 3 / 4, a pitch shorter than the row / frame it strides;  GNR_ERR_SHAPE: n < 1, a
 * dimension outside 1..16384, more than 2^31 - 1 groups of four output pixels;  text in gnr_last_error(). */
#define GNR_INGEST_MAX_DIM 16384
size_t gnr_ingest_tables_bytes(int dst_h, int dst_w);
int gnr_ingest_tables_host(int src_h, int src_w, int dst_h, int dst_w, void* tables_host);
int gnr_ingest_u8(const unsigned char* frames, int n, int src_h, int src_w, int channels, size_t row_pitch, size_t frame_pitch,
                  const void* tables_dev, float* out, int dst_h, int dst_w, void* stream);
const char* gnr_ingest_last_error(void);     /* alias of gnr_last_error() */

/* ---- frame metrics of a validation pass (csrc/gnr_metrics.hip) ---------------------------------------------------
 * The reference's PSNR_SSIM metric (network/metrics.py:14-30,40-84) for B full frames at once, all on the device:
 *   gt [B,h*w,3], preds[p] [B,h*w,3] for p < n_pred (`preds` is a HOST array of n_pred device pointers, n_pred in
 *   1..GNR_METRICS_MAX_PRED: pixel_colors_nr, pixel_colors_nr_fine), depth_pr [B,h*w], depth_gt [B,h,w], all float32.
 *   out: DEVICE float64 [B][2 * n_pred + 1] = psnr[n_pred], ssim[n_pred], depth_mae per scene.
 * PSNR: both images quantised as color_map_backward does (utils/base_utils.py:496-499: one fp32 multiply by 255, clip to
 *   [0,255], truncation to uint8), cropped by h_margin rows / w_margin columns on every side (the caller computes
 *   int(h * (1 - eval_margin_ratio)) // 2), 10 log10(255^2 / mse) with the squared differences summed as 64-bit integers
 *   (exact) and the rest in double;  mse == 0 -> +inf;  a non-finite gt / prediction value inside the crop -> NaN (SSIM too).
 * depth_mae: mean of the fp32 |depth_pr - depth_gt| over the UNCROPPED frame (metrics.py:79-83), summed in double.
 * SSIM (ssim != 0; otherwise NaN is written): skimage.metrics.structural_similarity(gt, pr, win_size=11, multichannel=True,
 *   data_range=255) on the quantised, cropped images: exact int32 window sums, S in double, the mean over the frame without
 *   its 5-pixel border, then over the three channels.  Needs a cropped frame of at least 11 x 11: GNR_ERR_SHAPE otherwise.
 * Every floating-point sum is taken in a fixed order (per-workgroup partials in the workspace, one second stage; no float
 * atomics): two calls return the same bits.  Stream-ordered, no allocation, no host synchronisation, no library state.
 * GNR_ERR_ARG: null pointer, n_pred outside 1..4;  GNR_ERR_SHAPE: B outside 1..65535, h or w < 1, h * w >= 2^31, margins
 * that leave no pixel, a crop below the SSIM window;  GNR_ERR_WORKSPACE: workspace_bytes below
 * gnr_frame_metrics_workspace_bytes() of the same arguments (0 for arguments the entry point refuses);  text in gnr_last_error(). */
#define GNR_METRICS_MAX_PRED 4
size_t gnr_frame_metrics_workspace_bytes(int B, int h, int w, int n_pred, int h_margin, int w_margin, int ssim);
int gnr_frame_metrics(const float* gt, const float* const* preds, int n_pred, const float* depth_pr, const float* depth_gt, int B, int h,
                      int w, int h_margin, int w_margin, int ssim, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward twins ------------------------------------------------------------------------
 * Parameter gradients are DETERMINISTIC: the kernels use no float atomics on them.  Points / rays are assigned to
 * wavefronts statically, every wavefront stores its partial sums into its own slot of a partial buffer inside the
 * caller-owned scratch / training workspace, and one reduction kernel per entry point adds the slots in slot order (in
 * double) into d_canonical / dtail.  Two calls on the same inputs return the same bits (the reference's CPU backward is
 * deterministic as well: ibrnet.py:497-504 + autograd).  The feature-map gradients (d_ray_feats, d_img_feats: a bilinear
 * scatter, like ATen's grid_sampler backward on a GPU) are accumulated with float atomics by default: their low bits depend on
 * the arrival order.  GNR_OPT_FEATURE_GRAD_FIXED (GnrScene.options of the backward call) makes them BIT-REPRODUCIBLE too: every
 * contribution is rounded once to a multiple of a launch-wide power-of-two quantum (2^-28 of the launch's largest upstream gradient,
 * found by an order-independent maximum) and added as a 64-bit integer (integer adds commute); a contribution more than 2^14 times the
 * upstream maximum is clamped and raises bit 3 of gnr_range_status.
 * Every entry point that produces feature-map gradients honours it (gnr_depth_mean_bwd, gnr_sample_volume_bwd,
 * gnr_render_chain_bwd); their workspaces are sized for either mode.  In the float mode the view kernels' scatter is BINNED (round 6,
 * csrc/gnr_bwd_scatter.inc): the per-(view, point) rows are parked in the training workspace and summed per feature-map pixel before
 * anything is added atomically (786 M -> ~40 M atomic dwords per 8-scene volume launch).  In the fixed-point mode the same rows are
 * summed as 64-bit integers (same rounding per contribution, same bits as the direct fixed-point scatter): no extra cost.
 * gnr_depth_mean_bwd: the backward of gnr_depth_mean_fwd (predict_mean_for_depth_loss, renderer.py:230-266,
 * consumed by DepthLoss, loss.py:87-144).  sample_volume and the per-view chain of the render passes follow below;
 * the render path's twin pairs (per-view chain, per-ray tail, compositing) follow further down.
 *   gnr_pack_weights_bwd: canonical blob -> transposed MFMA fragments [gnr_packed_bwd_floats()]
 *   gnr_depth_mean_bwd:   dmean [B,V,pn,2] -> d_canonical [gnr_canonical_weights_floats()] (ACCUMULATED:
 *                         mean_decoder.{0,2,4}.{weight,bias} entries, state-dict order) and
 *                         d_ray_feats [B,V,32,fh,fw] (overwritten; NULL to skip).  Needs gnr_prepare's
 *                         workspace (feature maps in channel-last form) and a separate scratch buffer of
 *                         gnr_depth_mean_bwd_workspace_bytes(scene) for the partial parameter gradients and the
 *                         channel-last feature gradient (required, also with d_ray_feats == NULL).            */
int gnr_packed_bwd_floats(void);
int gnr_pack_weights_bwd(const float* canonical_host, float* packed_bwd_host);
size_t gnr_depth_mean_bwd_workspace_bytes(const GnrScene* scene);
int gnr_depth_mean_bwd(const GnrScene* scene, const float* coords, int pn, const float* level_weights,
                       const float* level_weights_bwd, const float* dmean, float* d_canonical, float* d_ray_feats,
                       void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* sample_volume for training: the forward that also saves the per-view states (same values and speed as
 * gnr_sample_volume_fwd), and its backward in five stages (csrc/gnr_bwd.inc): bit 4 = attention / LayerNorm /
 * out_geometry_fc tail, bit 3 = geometry_fc + second cross-view reduction, bit 2 = second view loop (base_fc, vis_fc,
 * vis_fc2), bit 1 = hoisted base_fc.0 columns + first reduction, bit 0 = first view loop (decoder, prob_embed,
 * ray_dir_fc, neuray gate) + feature-map gradients.  `stages` = 0x1f runs all of it; partial masks exist for the staged
 * tests, which read the inter-stage gradients through gnr_train_workspace_layout().  d_canonical is ACCUMULATED
 * (state-dict order, coarse level); d_ray_feats / d_img_feats [B,V,32,fh,fw] are overwritten (NULL to skip).  The
 * training workspace and the regular workspace must survive untouched from the forward to the backward.              */
size_t gnr_sample_volume_train_workspace_bytes(const GnrScene* scene, int volume_res);
int gnr_train_workspace_layout(const GnrScene* scene, int volume_res, size_t* offsets_out9);
int gnr_sample_volume_fwd_train(const GnrScene* scene, const float* bbox_min, int volume_res, const float* level_weights,
                                float* sdf_out, void* workspace, size_t workspace_bytes, void* train_workspace,
                                size_t train_workspace_bytes, void* stream);
int gnr_sample_volume_bwd(const GnrScene* scene, int volume_res, const float* level_weights, const float* level_weights_bwd,
                          const float* canonical_weights_dev, const float* dvol, float* d_canonical, float* d_ray_feats,
                          float* d_img_feats, void* workspace, size_t workspace_bytes, void* train_workspace,
                          size_t train_workspace_bytes, int stages, void* stream);

/* Test tooling of the binned scatter (csrc/gnr_bwd_scatter.inc), in the style of gnr_debug_sample_order.
 * gnr_scatter_workspace_layout: byte offsets of the stage's buffers {rows, wts, key, cnt, cursor, list, nseg} inside a training
 *   workspace and, as the eighth entry, its number of rows N -- dn == 0: the volume's workspace at volume_res = n
 *   (gnr_sample_volume_train_workspace_bytes), else the workspace of a render pass of n rays x dn samples
 *   (gnr_render_chain_train_workspace_bytes).
 * gnr_debug_feature_scatter: the stage alone on caller-given device arrays rows [N][64], wts [N][4] (w00 w01 w10 w11), key [N]
 *   (N = B * tiles_per_scene * V * 16, row id = ((b * tiles_per_scene + tile) * V + v) * 16 + point; key = (b * V + v) * fh * fw +
 *   top-left tap pixel, or -1 for a dead row).  It clears the bin counts, counts the live keys (what the view kernel's atomics do
 *   in a backward), clears `raw` and then makes exactly a backward's launches: placement, k_scatter_gather, k_unpack_feat_grad.
 *   fixed != 0: the fixed-point mode with upmax_bits = the bits of the launch's largest upstream gradient.  path: 0 = the
 *   placement a backward takes at this feature-map size, 1 = the LDS placement (at most 38 400 pixels), 2 = k_scatter_scan +
 *   k_scatter_fill.  A key outside its own row's scene-view range [(b * V + v) * fh * fw, + fh * fw) is taken as -1 before
 *   anything consumes it, so no input indexes out of range; the taps of a row in the last column / row are the caller's to zero
 *   (the stage skips them there whatever their weight).
 *   Outputs: d_ray_feats / d_img_feats [B,V,32,fh,fw] (each nullable); raw = the channel-last buffer [B*V][fh*fw][64] (floats, or
 *   64-bit multiples of the quantum) of raw_bytes; status_out2 (device, two words): [0] = status bits (bit 3: a clamped
 *   contribution), [1] = the number of keys taken as -1.  gnr_debug_feature_scatter_bytes -> the bytes of `scratch` (and of `raw`);
 *   0 for a refused shape. */
int gnr_scatter_workspace_layout(const GnrScene* scene, int n, int dn, size_t* offsets_out8);
size_t gnr_debug_feature_scatter_bytes(int B, int V, int fh, int fw, int tiles_per_scene, size_t* raw_bytes);
int gnr_debug_feature_scatter(int B, int V, int fh, int fw, int tiles_per_scene, const float* rows, const float* wts, const int* key,
                              unsigned upmax_bits, int fixed, int path, float* d_ray_feats, float* d_img_feats, void* raw, size_t raw_bytes,
                              void* scratch, size_t scratch_bytes, unsigned* status_out2, void* stream);

/* Render path for training: the per-view chain of one render pass in both directions; the per-ray tail (renderer.py:90-108,
 * ibrnet.py:485-504) and NeuS alpha / compositing have their own twin pairs below; the ray geometry (S1-S3), the inverse-CDF
 * resampling and the sort (F1/F2) run in the forward kernels.  PyTorch autograd only connects the pairs with the losses.
 *   stats_out [B, rn*dn, 66] = mean(32) var(32) wbar n_valid_views (true scale); colors_out [B, rn*dn, 3]           */
size_t gnr_render_chain_train_workspace_bytes(const GnrScene* scene, int rn, int dn);
/*   depth == NULL: the coarse pass, sample_depth (render_ops.py:146-170) on the device (dn must be rays->dn, 3..64).
 *   depth != NULL: dn caller-given depths per ray, 3..128 (fine_depth_use_all, renderer.py:145-146: the fine pass renders the
 *   coarse and the resampled depths together); gnr_render_tail_fwd_train, gnr_ray_tail_dual_bwd and gnr_composite_bwd take the
 *   same range (the inverse-CDF resampler, fine_depth_out, at most 64).
 *   depth_out [B,rn,dn], pts_out [B,rn*dn,3], qdir_out [B,rn,3] (each nullable): the depths the pass used and its ray
 *   geometry (render_ops.py:4-39: sample points, normalised query directions) for the tail / compositing backward.  */
int gnr_render_chain_fwd_train(const GnrScene* scene, const GnrRays* rays, const float* depth, int dn, const float* level_weights,
                               float* stats_out, float* colors_out, float* depth_out, float* pts_out, float* qdir_out,
                               void* workspace, size_t workspace_bytes, void* train_workspace, size_t train_workspace_bytes,
                               void* stream);
int gnr_render_chain_bwd(const GnrScene* scene, int rn, int dn, const float* level_weights, const float* level_weights_bwd,
                         const float* dstats, const float* dcolors, float* d_canonical, float* d_ray_feats, float* d_img_feats,
                         void* workspace, size_t workspace_bytes, void* train_workspace, size_t train_workspace_bytes,
                         void* stream);

/* Per-ray tail of a training render pass (ibrnet.py:485-504: geometry_fc, positional encoding, 40-token attention,
 * LayerNorm, out_geometry_fc, clip, and the in-forward gradient of sdf w.r.t. the ray points, create_graph=True).
 * Forward: gnr_render_tail_fwd_train runs the inference tail kernel (tail + NeuS alpha + compositing) on the records
 * gnr_render_chain_fwd_train just left in `workspace` (call it right after that chain): out->colors_nr is the INPUT (the
 * chain's colours), every other non-null member of `out` is written as by gnr_render_by_depth_fwd.
 * Backward: with a = dL/d sdf and gamma = dL/d grad the gradients are those of  sum a*sdf + <gamma, grad>  =  a reverse
 * pass over the tail evaluated on dual numbers (value, derivative along gamma).  gnr_ray_tail_dual_bwd is its attention /
 * LayerNorm / out_geometry_fc core for a flat list of rays: g, gd [nrays*dn,16] value and tangent of geometry_fc's output,
 * a, nvalid [nrays*dn] -> gbar, gdbar [nrays*dn,16] and dtail [gnr_ray_tail_grad_floats()] = dWq, dWk, dWv, dWfc [16][16],
 * dLNw, dLNb [16], d w_eff [16], d b_eff (out_geometry_fc folded into one row; unfolded by the caller).  The two ELU
 * layers of geometry_fc around it: gnr_geo_dual_fwd / gnr_geo_dual_bwd below.                                        */
/* fine_depth_out [B,rn,rays->fdn] (nullable): this (coarse) pass's inverse-CDF resampling, sorted (render_ops.py:172-229,
 * renderer.py:146-148); rays->fine_u = the is_train draws, NULL = eval midpoints. */
int gnr_render_tail_fwd_train(const GnrScene* scene, const GnrRays* rays, const float* depth, int dn, const float* level_weights,
                              GnrRenderOut* out, float* fine_depth_out, void* workspace, size_t workspace_bytes,
                              void* train_workspace, size_t train_workspace_bytes, void* stream);
int gnr_ray_tail_grad_floats(void);
/* geometry_fc (86 -> 64 -> 16, two ELUs; ibrnet.py:488-489) on dual numbers, around gnr_ray_tail_dual_bwd.  canonical_dev =
 * the level's parameters in state-dict order on the device; stats [P,66] (mean 32, var 32, wbar, n_valid), pts, gamma [P,3].
 * fwd: g, gd [P,16] = value / derivative along gamma of geometry_fc's output.  bwd: gbar, gdbar [P,16] -> dstats [P,66]
 * (overwritten) and the gradients of geometry_fc.{0,2}.{weight,bias} ACCUMULATED into d_canonical (state-dict order).   */
/* fwd runs on the f16 matrix cores like the backward's per-point half (16 points as the columns of a chained fp16-pair MFMA, fragments
 * packed per call into caller-owned scratch of gnr_geo_dual_fwd_workspace_bytes() bytes; a call whose outputs come out non-finite -- a
 * weight or an operand beyond the fp16 range -- is recomputed by the fp32 kernel launched behind it); GNR_OPT_GEO_DUAL_FP32: the fp32 FMA
 * kernel alone (scratch may then be NULL). */
size_t gnr_geo_dual_fwd_workspace_bytes(void);
int gnr_geo_dual_fwd(const float* canonical_dev, const float* stats, const float* pts, const float* gamma, float* g, float* gd,
                     int P, void* scratch, size_t scratch_bytes, unsigned options, void* stream);
/* bwd runs as two kernels (the per-point reverse pass -- 16 points as the columns of a chained fp16-pair MFMA, its fragments packed per
 * call from canonical_dev -- then the weight-gradient outer products over the points on the matrix cores) with the per-point adjoints
 * between them (288 floats per point), the fragment image (64 KB) and the partial weight gradients in caller-owned scratch of
 * gnr_geo_dual_bwd_workspace_bytes(P) bytes. */
size_t gnr_geo_dual_bwd_workspace_bytes(int P);
int gnr_geo_dual_bwd(const float* canonical_dev, const float* stats, const float* pts, const float* gamma, const float* gbar,
                     const float* gdbar, float* dstats, float* d_canonical, int P, void* scratch, size_t scratch_bytes, unsigned options,
                     void* stream);
/* Backward of NeuS alpha + compositing (aggregate_net.py:105-121, render_ops.py:72-80, renderer.py:110-123) for a flat list
 * of rays, forward values taken from the tensors the forward wrote: sdf [nrays*dn], grad, col [nrays*dn,3], depth
 * [nrays*dn], qdir [nrays,3].  Upstream: dpix [nrays,3]; ddepth [nrays], wgerr [nrays] (d L / d sum_k (|grad_k|-1)^2 of the
 * ray), dalpha, dhit [nrays*dn] may be null.  Out: a_out = dL/d sdf, gamma_out = dL/d grad (the upstreams of
 * gnr_ray_tail_dual_bwd), dcol_out, dvar_out[0] = dL/d deviation_network.variance (all overwritten).
 * scratch: gnr_composite_bwd_workspace_bytes(nrays) / gnr_ray_tail_dual_bwd_workspace_bytes() bytes, caller-owned (the
 * per-wavefront partial sums of the parameter gradients).  `options` of gnr_ray_tail_dual_bwd / gnr_geo_dual_fwd / gnr_geo_dual_bwd: GNR_OPT_* (these
 * entry points take no GnrScene): GNR_OPT_POISON_PARTIALS, and GNR_OPT_GEO_DUAL_FP32 for gnr_geo_dual_fwd / gnr_geo_dual_bwd.                 */
size_t gnr_composite_bwd_workspace_bytes(int nrays);
int gnr_composite_bwd(const float* level_weights, const float* sdf, const float* grad, const float* col, const float* depth,
                      const float* qdir, const float* dpix, const float* ddepth, const float* wgerr, const float* dalpha,
                      const float* dhit, float* a_out, float* gamma_out, float* dcol_out, float* dvar_out, int nrays, int dn,
                      void* scratch, size_t scratch_bytes, void* stream);
size_t gnr_ray_tail_dual_bwd_workspace_bytes(void);
int gnr_ray_tail_dual_bwd(const float* level_weights, const float* g, const float* gd, const float* a, const float* nvalid,
                          float* gbar, float* gdbar, float* dtail, int nrays, int dn, void* scratch, size_t scratch_bytes,
                          unsigned options, void* stream);

/* ---- host helper ---------------------------------------------------------------------------
 * The first k entries of torch.randperm(n) on the CPU generator, bit-exact, in O(k + n/624) instead of n random-access swaps:
 * the reference draws the depth-loss pixels as torch.randperm(h*w)[:8192] (src/nr/network/renderer.py:222-228), 5-15 ms per
 * scene on the host.  torch_cpu_rng_state = the bytes of torch.get_rng_state() (5056), advanced in place exactly as
 * torch.randperm(n) would advance the generator; out[k] int64.  Returns GNR_ERR_SHAPE for state layouts / sizes it does not
 * know (the caller then falls back to torch.randperm).  No device work.                                          */
int gnr_host_randperm_prefix(unsigned char* torch_cpu_rng_state, long long state_bytes, long long n, int k, long long* out);

/* ---- grasp post-processing on the device -------------------------------------------------
 * Replaces the reference planner's `process` + `select` (src/nr/main.py:23-57, 60-84), which run
 * scipy.ndimage (gaussian_filter sigma=1 mode='nearest'; binary_dilation iterations=2 with mask;
 * maximum_filter size=4) on the host for every plan.  Bit-exact with scipy: fp64 accumulation in
 * scipy's order, fp32 rounding after every Gaussian axis.
 *   tsdf, qual, width [B,R,R,R], rot [B,4,R,R,R]  (outputs of sample_volume / the grasp head)
 *   qual_out [B,R,R,R]      processed quality volume                        (main.py:41-55)
 *   count [B]               selected grasps per scene (may exceed max_n: only the first max_n are stored)
 *   index [B,max_n,3] (i,j,k), score [B,max_n], quat [B,max_n,4] (x,y,z,w as stored in rot),
 *   width_out [B,max_n]     in np.argwhere order                            (main.py:70-84)              */
#define GNR_GAUSS_MAX_RADIUS 16
typedef struct GnrSelectParams {
    int gauss_radius;                          /* int(4*sigma + 0.5)                                    */
    double gauss_w[GNR_GAUSS_MAX_RADIUS + 1];  /* w[k] = exp(-k^2/(2 sigma^2)) / sum, k = 0..radius     */
    float tsdf_thres_high, tsdf_thres_low;     /* planner: 0, -0.85 (main.py:93-94)                     */
    float min_width, max_width;                /* 1.33, 9.33 (main.py:29-30)                            */
    float threshold;                           /* 0.90 (main.py:60)                                     */
    int dilate_iterations;                     /* 2 (main.py:48)                                        */
    int max_filter_size;                       /* 4 (main.py:60)                                        */
} GnrSelectParams;
size_t gnr_grasp_select_workspace_bytes(int B, int R);
int gnr_grasp_select_fwd(const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                         const GnrSelectParams* params, float* qual_out, int* count, int* index, float* score,
                         float* quat, float* width_out, int max_n, void* workspace, size_t workspace_bytes, void* stream);
const char* gnr_post_last_error(void);       /* alias of gnr_last_error() */

/* ---- the real-robot route (src/nr/utils/grasp_utils.py:40-151, draw_utils.py:355-382) ----
 * gnr_grasp_select_v2_fwd: gnr_grasp_select_fwd with three more parameters; every argument, output and
 * layout is that call's, and with tsdf_thres_outside == select.tsdf_thres_high, GNR_SELECT_ORDER_INDEX and
 * top_k == 0 so is every bit (gnr_grasp_select_fwd is this call with those values).
 *   tsdf_thres_outside   outside = tsdf > tsdf_thres_outside, while may_change stays
 *                        !(tsdf_thres_low < tsdf < tsdf_thres_high): the three thresholds of
 *                        grasp_utils.process (0.1 / -0.1 / -1, grasp_utils.py:59-60)
 *   order                GNR_SELECT_ORDER_INDEX: np.argwhere order.  GNR_SELECT_ORDER_SCORE: descending
 *                        score, equal scores by ascending linear voxel index -- sim_grasp's
 *                        np.argsort(scores)[::-1][:top_k] (grasp_utils.py:105), except that numpy leaves the
 *                        order of tied scores unspecified (argsort's default sort is not stable, and [::-1]
 *                        would reverse a stable one): on ties this order is this library's, not numpy's.
 *                        The ranking is over ALL survivors (non-maximum suppression keeps every voxel of a
 *                        plateau: up to R^3), never over the first max_n in index order.  R <= 64
 *                        (GNR_SELECT_SCORE_MAX_R: 2^18 voxels per scene, the limit of the render path's
 *                        sample order); a larger R is refused.  GNR_SELECT_ORDER_INDEX keeps R <= 256.
 *   top_k                rows stored per scene = min(count, top_k, max_n); 0: as many as max_n
 *   count [B]            ALL survivors per scene in either order (may exceed top_k and max_n)            */
#define GNR_SELECT_ORDER_INDEX 0
#define GNR_SELECT_ORDER_SCORE 1
#define GNR_SELECT_SCORE_MAX_R 64
typedef struct GnrSelectParamsV2 {
    GnrSelectParams select;
    float tsdf_thres_outside;
    int order;                                 /* GNR_SELECT_ORDER_*                                    */
    int top_k;
} GnrSelectParamsV2;
size_t gnr_grasp_select_v2_workspace_bytes(int B, int R, int order);
int gnr_grasp_select_v2_fwd(const float* tsdf, const float* qual, const float* rot, const float* width, int B, int R,
                            const GnrSelectParamsV2* params, float* qual_out, int* count, int* index, float* score,
                            float* quat, float* width_out, int max_n, void* workspace, size_t workspace_bytes, void* stream);
/* gnr_surface_points_fwd: extract_surface_points_from_volume (draw_utils.py:355-377) for B volumes in one
 * launch sequence: per scene the voxels with lo < vol < hi in np.nonzero order (ascending linear index).
 *   vol [B,R,R,R], R <= 256
 *   count [B]               voxels in range per scene (may exceed max_n: only the first max_n are stored)
 *   index [B,max_n,3]       (i,j,k) int32
 *   points [B,max_n,3]      float64, index * scale (open3d's PointCloud.scale about the origin)
 *   colors [B,max_n,3]      float32: `color` for every point (GNR_SURFACE_COLOR_FIXED), or the value map of the
 *                           reference's color=None branch (GNR_SURFACE_COLOR_VALUE, draw_utils.py:364-370) in
 *                           float32, v = vol at the voxel:  m = (a + b) / 2;  r = v <= m ? v - a : -v + b;
 *                           g = v <= m ? 0 : 1 - r;  b = v <= m ? 1 - r : 0
 * Entries beyond min(count[b], max_n) are undefined.                                                   */
#define GNR_SURFACE_COLOR_FIXED 0
#define GNR_SURFACE_COLOR_VALUE 1
typedef struct GnrSurfaceParams {
    float lo, hi;                              /* (-0.2, 0.2) (grasp_utils.py:149)                      */
    int color_mode;                            /* GNR_SURFACE_COLOR_*                                   */
    float color[3];                            /* (0, 0, 1) (draw_utils.py:355)                         */
    float bound_a, bound_b;                    /* (-1, 1) (draw_utils.py:355)                           */
    double scale;                              /* 0.3 / 40 (draw_utils.py:355)                          */
} GnrSurfaceParams;
size_t gnr_surface_points_workspace_bytes(int B, int R);
int gnr_surface_points_fwd(const float* vol, int B, int R, const GnrSurfaceParams* params, int* count, int* index,
                           double* points, float* colors, int max_n, void* workspace, size_t workspace_bytes, void* stream);

/* Rows of a gradient volume (the entry point above the render passes) at the voxels of a surface cloud:
 *   out[b,r,:] = grad[b, index[b,r]]  for r < min(count[b], max_points);  grad [B,R,R,R,3], index / count as the surface-point call
 *   wrote them for the same max_points, out [B,max_points,3] float32.  Rows beyond that are left untouched.  1 <= R <= 256. */
int gnr_surface_gradient_fwd(const float* grad, const int* index, const int* count, int B, int R, int max_points,
                             float* out /*[B,max_points,3]*/, void* stream);

/* gnr_surface_mesh_fwd: an indexed triangle mesh of the iso-surface vol = iso of B volumes [B,R,R,R], 2 <= R <= 256 (predicted SDF
 * volumes and fused TSDF grids alike), by naive surface nets.  No reference counterpart; tests/mesh_reference.py is the same
 * statement in numpy and the call produces its bits.
 *   inside     voxel p is inside iff vol[p] < iso, compared in float32 (a value equal to iso is outside).
 *   cells      cell q in [0,R-2]^3 has the corners q + {0,1}^3 and is active iff they are not all on one side.
 *   vertex     of an active cell: its 12 edges in the order  for a in (0,1,2): b, c = (a+1)%3, (a+2)%3; for dc in (0,1): for db in (0,1):
 *              from p0 = q + db e_b + dc e_c to p1 = p0 + e_a.  Where the ends differ in the inside test: t = ((double)iso - v0) / (v1 - v0),
 *              crossing point p0 + t e_a in voxel-index units.  The points are summed sequentially in that order per component,
 *              mean = sum / n, vertex = origin + mean * scale (a multiplication, then an addition), all float64.
 *              Vertex order: ascending cell index x (R-1)^2 + y (R-1) + z.
 *   faces      edge (p, a) from voxel p to p + e_a is interior iff p_a <= R-2, 1 <= p_b <= R-2 and 1 <= p_c <= R-2.  A sign-changing
 *              interior edge gives one quad over the four cells around it, named by minimum corner: q0 = p - e_b - e_c, q1 = p - e_c,
 *              q2 = p, q3 = p - e_b.  p inside (vol rises along +a): triangles (q0,q1,q2), (q0,q2,q3); otherwise (q0,q2,q1), (q0,q3,q2);
 *              entries are the cells' vertex rows, int32.  Face order: ascending (voxel index of p) * 3 + a, a quad's two triangles
 *              adjacent.  Triangle normals point towards increasing vol: out of the object for a signed distance.
 *   gradient   optional: with grad [B,R,R,R,3] float32, gradient[vertex] = the mean over the same edges in the same order of
 *              g0 + t (g1 - g0), float64 per component, rounded once to float32; not normalised.  grad and gradient are both
 *              given or both NULL.
 *   count [B,2]              vertices and triangles per scene: the true totals, also beyond max_v / max_f
 *   vertices [B,max_v,3]     float64;   faces [B,max_f,3] int32;   gradient [B,max_v,3] float32
 * Rows beyond a cap and rows beyond the count are left untouched; a face names the true row of a vertex even when that row is beyond
 * max_v.  At most (R-1)^3 vertices and 6 (R-1) (R-2)^2 triangles per scene.  1 <= B <= 65535, max_v, max_f >= 1; iso, scale and origin
 * finite.  The volume is finite (sample_volume clips to [-1,1]); the result on a NaN or an infinity is undefined.
 * Asynchronous on `stream`, no atomics, no allocation, no synchronisation (it can be captured in a graph); a refused call has
 * launched nothing.  The workspace need not be cleared between calls.                                                       */
typedef struct GnrMeshParams {
    float iso;
    double scale;                              /* 0.3 / 40: the surface cloud's                         */
    double origin[3];
} GnrMeshParams;
size_t gnr_surface_mesh_workspace_bytes(int B, int R);
int gnr_surface_mesh_fwd(const float* vol, const float* grad /*NULL: no normals*/, int B, int R, const GnrMeshParams* params,
                         int* count /*[B,2]: vertices, triangles*/, double* vertices /*[B,max_v,3]*/, int* faces /*[B,max_f,3]*/,
                         float* gradient /*[B,max_v,3], NULL iff grad is*/, int max_v, int max_f, void* workspace, size_t workspace_bytes,
                         void* stream);

/* gnr_volume_raycast_fwd: depth (and gradient) images of the iso-surface vol = iso of B volumes [B,R,R,R], 2 <= R <= 256, seen from V
 * pinhole cameras each (poses: world->camera, OpenCV axes), one ray through every integer pixel centre (u, v).  No reference
 * counterpart; tests/raycast_reference.py is the same statement in numpy and the call produces its bits.  poses and Ks convert to
 * float64 before the first operation; everything below is float64, single correctly rounded operations in the order written.
 *   ray        dc = ((u - cx) / fx, (v - cy) / fy, 1);  eye_a = -((R[0][a] t[0] + R[1][a] t[1]) + R[2][a] t[2]);
 *              dw_a = (R[0][a] dc_x + R[1][a] dc_y) + R[2][a].  The parameter s of eye + s dw is camera-z depth in metres.
 *   index      e = (eye - origin) / scale, d = dw / scale per component: lattice point i sits at world origin + i * scale (the mesh's
 *              convention; a caller with voxel centres passes origin = bbox_min + 0.5 * scale).
 *   box        slabs against [0, R-1] per axis: lo_a = min((0 - e_a) / d_a, ((R-1) - e_a) / d_a), hi_a likewise with max.  An axis with
 *              d_a == 0 imposes no bound when 0 <= e_a <= R-1 and makes the ray miss otherwise (nothing rests on inf / NaN
 *              arithmetic).  s0 = max(lo_x, lo_y, lo_z, near_s), s1 = min(hi_x, hi_y, hi_z, far_s); a miss unless s0 < s1 (and s1 finite).
 *   march      ds = step / sqrt((d_x d_x + d_y d_y) + d_z d_z): `step` voxels of path per sample.  n = ceil((s1 - s0) / ds), at most
 *              ceil(sqrt(3) (R-1) / step) + 1 (a bound that holds for every ray in exact arithmetic; it ends the loop on cameras that hold
 *              no numbers).  s_k = min(s0 + (double)k * ds, s1), k = 0..n;  f(s) = trilinear(vol, e + s * d) - (double)iso.
 *   trilinear  base b = clamp(floor(p), 0, R-2) per axis, t = p - b; the eight float32 corners convert to float64; lerp along z, then y,
 *              then x, each a + t * (b - a).
 *   hit        the first k >= 1 with f(s_{k-1}) >= 0 and f(s_k) < 0: outside -> inside, inside being the mesh's vol < iso.  A ray that
 *              starts inside does not hit until it has left and entered again.
 *   refine     `bisections` halvings of [A, B] = [s_{k-1}, s_k]: m = 0.5 * (A + B), f(m) < 0 replaces B, otherwise A; then one secant
 *              step s* = A + (B - A) * (fA / (fA - fB)).  depth = (float)s*; a miss gives 0, gnr_tsdf_integrate's "no depth".
 *   gradient   optional: with grad [B,R,R,R,3] float32, gradient[pixel] = the same trilinear form per component at e + s* d, rounded
 *              once to float32, not normalised (the mesh's rule); 0 on a miss.  grad and gradient are both given or both NULL.
 *   vol [B,R,R,R];  poses [B,V,3,4];  Ks [B,V,3,3];  depth [B,V,h,w];  gradient [B,V,h,w,3].  Every pixel of depth (and of gradient)
 *   is written, nothing else is.
 * 1 <= B <= 65535, V >= 1, h, w >= 1 (at most 2^28 tiles of 8 x 8 pixels), 0 <= bisections <= 32; scale, step finite and > 0, and step
 * large enough that the march's bound is at most GNR_RAYCAST_MAX_SAMPLES; iso, origin finite; near_s >= 0, far_s > near_s (far_s may
 * be infinite).  The result on a volume that holds a NaN or an infinity is undefined (but no access leaves the volume).
 * Asynchronous on `stream`, no atomics, no workspace, no allocation, no synchronisation (it can be captured in a graph); a refused
 * call has launched nothing.                                                                                                  */
#define GNR_RAYCAST_MAX_SAMPLES 65536
typedef struct GnrRaycastParams {
    int B, V, h, w, R, bisections;
    float iso;
    double scale, step, near_s, far_s;
    double origin[3];
} GnrRaycastParams;
int gnr_volume_raycast_fwd(const GnrRaycastParams* params, const float* vol /*[B,R,R,R]*/, const float* grad /*[B,R,R,R,3] or NULL*/,
                           const float* poses /*[B,V,3,4]*/, const float* Ks /*[B,V,3,3]*/, float* depth /*[B,V,h,w]*/,
                           float* gradient /*[B,V,h,w,3], NULL iff grad is*/, void* stream);

/* gnr_surface_color_points_fwd / gnr_surface_color_pixels_fwd: view colours of surface points of B volumes [B,R,R,R] -- each point takes
 * the colour of the V source images [B,V,3,H,W] it is seen in, weighted by how squarely it faces each camera, with visibility decided
 * by the volume itself (a march from the point towards the eye).  One kernel body; the two entry points differ only in where a point
 * comes from: rows of a point array (the surface cloud, the mesh's vertices), or the pixels of depth images of gnr_volume_raycast_fwd
 * (the result is then an image-based rendering of the scene from those cameras).  No reference counterpart;
 * tests/surface_color_reference.py is the same statement in numpy and the calls produce its bits.  vol, images, poses, Ks, depth, iso and
 * fill convert to float64 before the first operation; everything below is float64, single correctly rounded operations in the order
 * written.  Lattice point i of the volume sits at world origin + i * scale (the ray cast's convention).
 *   cameras    eye_a and the pixel ray dw_a of a camera exactly as in gnr_volume_raycast_fwd;  e_a = (eye_a - origin_a) / scale.
 *   point      points:  x_a = point_offset_a + points[b,r,a] for r < min(count[b * count_stride], max_n); other rows are left untouched.
 *              pixels:  s = depth[b,c,y,x];  s <= 0 (the ray cast's miss) gives fill, weight 0, views 0;  otherwise
 *                       x_a = eye'_a + s * dw'_a with eye', dw' of the target camera c (cam_poses, cam_Ks) through pixel (x, y).
 *              p_a = (x_a - origin_a) / scale.
 *   normal     from the volume:  g_a = T(p + 0.5 u_a) - T(p - 0.5 u_a), u_a the unit vector of axis a and T the trilinear value of
 *              gnr_volume_raycast_fwd (base clamp(floor(.), 0, R-2); z, then y, then x);  n2 = (g_x g_x + g_y g_y) + g_z g_z;
 *              n2 == 0: no view contributes.
 *   views      v = 0 .. V-1 in this order, each with its pose (R | t) and K:
 *     project    pc_a = ((R[a][0] x_0 + R[a][1] x_1) + R[a][2] x_2) + t_a;  skip unless pc_z > 0.
 *                u = pc_x * fx / pc_z + cx, v = pc_y * fy / pc_z + cy (pixel centres are integers);  skip unless 0 <= u <= W-1 and
 *                0 <= v <= H-1.
 *     facing     q_a = e_a - p_a;  L = sqrt((q_x q_x + q_y q_y) + q_z q_z);  skip if L == 0;  d_a = q_a / L;
 *                c = ((g_x d_x + g_y d_y) + g_z d_z) / sqrt(n2);  skip unless c > cos_min.
 *     occlusion  samples s_k = bias + (double)k * step, k = 0, 1, .., while s_k < L and k < nmax = ceil(sqrt(3) (R-1) / step) + 1 (the
 *                ray cast's bound), at p + s_k d per component.  The first sample with a component outside [0, R-1] ends the march:
 *                visible.  A sample with T - (double)iso < 0 ends it: occluded, the view is skipped.  Out of samples: visible.
 *     colour     bilinear tap of images[b,v,ch] at (u, v): base clamp(floor(.), 0, size-2) per axis, t = coordinate - base; lerp along
 *                x in both rows, then along y, each a + t * (b - a).  acc_ch += c * colour_ch;  Wsum += c;  views |= 1 << v.
 *   result     colors_ch = (float)(acc_ch / Wsum) when Wsum > 0, else fill_ch;  weight = (float)Wsum;  views: the bit mask.
 * 1 <= B <= 65535, 1 <= V <= 32 (the mask), H, W >= 2, 2 <= R <= 256, max_n >= 1, count_stride >= 1 (2 for the mesh's [B,2] counts);
 * Vc, hc, wc >= 1 (at most 2^28 tiles of 8 x 8 pixels); scale, step finite and > 0, step large enough that nmax is at most
 * GNR_RAYCAST_MAX_SAMPLES; bias finite and >= 0; iso, origin, point_offset, cos_min, fill finite.  Results on a volume or images that
 * hold a NaN or an infinity are undefined, but no access leaves the volume or an image whatever the inputs hold.
 * Asynchronous on `stream`, no atomics, no workspace, no allocation, no synchronisation (they can be captured in a graph); a refused
 * call has launched nothing.                                                                                                  */
typedef struct GnrSurfaceColorParams {
    int B, V, H, W, R;
    float iso;
    double scale;
    double origin[3];
    double point_offset[3];                    /* points mode: the cloud and the mesh live in a frame with origin 0 */
    double step, bias, cos_min;                /* 0.5 and 1.5 voxels, 0                                              */
    float fill[3];                             /* the colour of a point no view contributes to                       */
} GnrSurfaceColorParams;
int gnr_surface_color_points_fwd(const GnrSurfaceColorParams* params, const float* vol /*[B,R,R,R]*/, const double* points /*[B,max_n,3]*/,
                                 const int* count /*[B * count_stride]*/, int count_stride, int max_n, const float* images /*[B,V,3,H,W]*/,
                                 const float* poses /*[B,V,3,4]*/, const float* Ks /*[B,V,3,3]*/, float* colors /*[B,max_n,3]*/,
                                 float* weight /*[B,max_n]*/, int* views /*[B,max_n]*/, void* stream);
int gnr_surface_color_pixels_fwd(const GnrSurfaceColorParams* params, const float* vol /*[B,R,R,R]*/, const float* depth /*[B,Vc,hc,wc]*/,
                                 const float* cam_poses /*[B,Vc,3,4]*/, const float* cam_Ks /*[B,Vc,3,3]*/, int Vc, int hc, int wc,
                                 const float* images /*[B,V,3,H,W]*/, const float* poses /*[B,V,3,4]*/, const float* Ks /*[B,V,3,3]*/,
                                 float* colors /*[B,Vc,hc,wc,3]*/, float* weight /*[B,Vc,hc,wc]*/, int* views /*[B,Vc,hc,wc]*/, void* stream);

/* gnr_hand_clearance_fwd: the clearance of a parallel-jaw hand at the ranked grasps of B volumes [B,R,R,R] -- per grasp the smallest
 * value of the volume over a lattice of samples of the hand's four boxes, once with the hand at the grasp and once over everything the
 * boxes pass through while the hand comes in from `approach` metres back along its own z (execute_grasp's pre-grasp pose,
 * gd/simulation.py:369-402, answered from the volume instead of physics).  No reference counterpart; tests/hand_reference.py is the same
 * statement in numpy and the call produces its bits.  vol, quat and width convert to float64 before the first operation; everything
 * below is float64, single correctly rounded operations in the order written.
 *   frame      the grasp frame of gd/vis.py's draw_grasp: z the approach (the fingers point along +z), y the closing direction, x the
 *              hand's thickness.  pos [B,max_n,3] float64 is in lattice units: voxel (i,j,k)'s value sits at position (i,j,k) (a
 *              selection's `index`, the cloud's points / scale).  Hand-local metres go to lattice units by division by `scale`.
 *   width      wv = opening / scale when opening >= 0 (one opening for every grasp), else (double)width[b,r] (voxels, a selection's);
 *              wv = fmin(fmax(wv, 0), (double)R) (fmax drops a NaN);  w = wv * scale;  hw = 0.5 * w.
 *   boxes      with h = height, f = finger_width, t = tail_length, d = depth, as (lo, extent) per axis, in this order:
 *                left finger   x (-0.5 h, h)   y (-hw - f, f)    z (-f, d + f)
 *                right finger  x (-0.5 h, h)   y (hw, f)         z (-f, d + f)
 *                palm          x (-0.5 h, h)   y (-hw, w)        z (-f, f)
 *                tail          x (-0.5 h, h)   y (-0.5 f, f)     z (-t - f, t)
 *              (draw_utils.draw_gripper_o3d's boxes under visualize_grasping_3d's y_ccw_90: its X is this z, its Z this -x).
 *   samples    cell = spacing * scale.  Per box and axis a with extent e:  n_a = fmax(2, ceil(e / cell) + 1), step_a = e / (n_a - 1),
 *              coordinates lo_a + (double)i * step_a, i = 0 .. n_a-1.  Along z the lattice continues backwards: i = -m .. -1 with
 *              m = ceil(approach / step_z) (approach == 0: m = 0).  Samples with i_z >= 0 are the hand AT THE GRASP, all samples the hand
 *              ON ITS APPROACH.  The ordinal of a sample counts all samples: box, then i_x, then i_y, then i_z ascending from -m.
 *   pose       q = (double)quat[b,r] (x, y, z, w);  n = fmax(sqrt(((x x + y y) + z z) + w w), 1e-12);  each component / n;  the matrix
 *              M = [[1 - 2 (y y + z z), 2 (x y - z w), 2 (x z + y w)], [2 (x y + z w), 1 - 2 (x x + z z), 2 (y z - x w)],
 *                   [2 (x z - y w), 2 (y z + x w), 1 - 2 (x x + y y)]]  (scipy's as_matrix; every product and sum as bracketed).
 *   position   of the local sample l:  p_a = pos_a + ((M[a][0] l_x + M[a][1] l_y) + M[a][2] l_z) / scale.  A sample with a component
 *              outside [0, R-1] (or not a number) is skipped: nothing is known there.  The others take the trilinear value T of
 *              gnr_volume_raycast_fwd (base clamp(floor(.), 0, R-2); z, then y, then x).
 *   result     per set (at the grasp: column 0; on the approach: column 1):  inside = the number of samples taken;  worst = the
 *              ordinal of the first sample in ordinal order whose T is the smallest (np.argmin: -0.0 and 0.0 tie), -1 when inside
 *              is 0;  clearance = (float)fmin(T at worst, free) with free = 1.0, the volume's upper clip; 1.0 when inside is 0.
 *   rows       r < min(count[b * count_stride], top_k > 0 ? top_k : max_n, max_n); the other rows are left untouched.
 * 1 <= B <= 65535, 2 <= R <= 256, max_n >= 1, count_stride >= 1, top_k >= 0; height, finger_width, tail_length, depth, spacing and
 * scale finite and > 0; approach finite and >= 0; opening finite. The number of samples of a grasp whose width is R voxels
 * (the most any row can have) must be at most GNR_HAND_MAX_SAMPLES.  Every loop is bounded by the parameters: no content of pos, quat,
 * width or count ends one later or moves an access out of the volume.  Results on a volume that holds a NaN are undefined.
 * Asynchronous on `stream`, no atomics, no workspace, no allocation, no synchronisation (it can be captured in a graph); a refused
 * call has launched nothing.                                                                                                  */
#define GNR_HAND_MAX_SAMPLES 4194304
typedef struct GnrHandParams {
    double height, finger_width, tail_length, depth;   /* metres: 0.004, 0.004, 0.04, 0.05 (the viewer's hand) */
    double opening;                                    /* metres; < 0: each grasp's own width                  */
    double spacing;                                    /* voxels between samples at most: 0.5                  */
    double approach;                                   /* metres: 0.05; 0: no sweep                            */
    double scale;                                      /* metres per voxel                                     */
} GnrHandParams;
int gnr_hand_clearance_fwd(const GnrHandParams* params, const float* vol /*[B,R,R,R]*/, const double* pos /*[B,max_n,3]*/,
                           const float* quat /*[B,max_n,4]*/, const float* width /*[B,max_n], voxels*/, const int* count /*[B * count_stride]*/,
                           int count_stride, int B, int R, int max_n, int top_k, float* clearance /*[B,max_n,2]*/, int* worst /*[B,max_n,2]*/,
                           int* inside /*[B,max_n,2]*/, void* stream);

/* gnr_finger_closure_fwd: where the two fingers of that hand stop when it closes on the volume, at the same rows -- the third step of
 * execute_grasp (gd/simulation.py:404, `gripper.move(0.0)`, and check_success, :465-469) answered from the volume.  The frame, `width`,
 * `pose`, `position`, `rows` and the trilinear value T are gnr_hand_clearance_fwd's, as are cell = spacing * scale and hw; tail_length
 * and approach are checked and not used.  tests/closure_reference.py is the same statement in numpy and the call produces its bits.
 *   pads       each finger's inner face carries pad rays over x in [-h/2, h/2] and z in [0, depth]:  n_x = fmax(2, ceil(height / cell) + 1),
 *              n_z = fmax(2, ceil(depth / cell) + 1), step = extent / (n - 1), l_x = -0.5 h + (double)i_x * step_x, l_z = (double)i_z *
 *              step_z.  The ordinal of a ray is i_x * n_z + i_z.
 *   travel     finger 0 starts at l_y = -hw and moves towards +y, finger 1 at +hw towards -y, both to the centre plane at the latest:
 *              n_y = fmax(1, ceil(hw / cell)), ds = hw / n_y, t_k = fmin((double)k * ds, hw) for k = 0 .. n_y;  after a travel of t:
 *              u = hw - t, l_y = -u (finger 0) or u (finger 1).  f(t) = value - level, where value is T at the position of (l_x, l_y, l_z)
 *              when every component of it lies in [0, R-1] and 1.0 (free) elsewhere: a finger outside the lattice touches nothing.
 *   ray        f(t_0) < 0: the pad starts inside, t* = 0.  Else the first k >= 1 with f(t_{k-1}) >= 0 and f(t_k) < 0 gives the bracket
 *              [A, B] = [t_{k-1}, t_k];  `bisections` times: m = 0.5 * (A + B), f(m) < 0 ? B = m : A = m (with their f's);  then
 *              t* = A + (B - A) * (fA / (fA - fB)) (gnr_volume_raycast_fwd's refinement).  No such k: the ray has no contact.
 *   finger     T_c = the smallest t* of its rays, contact_c = the lowest ordinal that attains it;  no ray with a contact: T_c = hw,
 *              contact_c = -1.
 *   cosine     at the position p of ray contact_c after a travel of T_c, with T's base corners c_xyz and t's, c00 .. c11 its z-lerped
 *              edges and c0, c1 its y-lerped faces:  g_x = c1 - c0;  g_y = e0 + t_x * (e1 - e0) with e0 = c01 - c00, e1 = c11 - c10;
 *              g_z = d0 + t_x * (d1 - d0) with d0 = d00 + t_y * (d01 - d00), d1 = d10 + t_y * (d11 - d10), d00 = c001 - c000 and
 *              likewise.  a = column 1 of M;  dot = (g_x a_0 + g_y a_1) + g_z a_2;  norm = fmax(sqrt((g_x g_x + g_y g_y) + g_z g_z), 1e-12);
 *              cos_0 = -dot / norm, cos_1 = dot / norm (1: the surface faces the finger squarely);  0 without a contact.
 *   result     travel[b,r,c] = (float)T_c (metres), cosine[b,r,c] = (float)cos_c, contact[b,r,c], closed[b,r] = (float)((hw - T_0) +
 *              (hw - T_1)): the width of the closed hand in metres.
 * The limits of gnr_hand_clearance_fwd, refused with its texts; level finite; 0 <= bisections <= 16; the volume reads of a grasp whose
 * width is R voxels, 2 n_x n_z (n_y + 1 + bisections + 2), must be at most GNR_HAND_MAX_SAMPLES.  Every loop is bounded by the
 * parameters; results on a volume that holds a NaN are undefined.  Asynchronous on `stream`, no atomics, no workspace, no allocation,
 * no synchronisation (it can be captured in a graph); a refused call has launched nothing.                                    */
int gnr_finger_closure_fwd(const GnrHandParams* params, double level, int bisections, const float* vol /*[B,R,R,R]*/,
                           const double* pos /*[B,max_n,3]*/, const float* quat /*[B,max_n,4]*/, const float* width /*[B,max_n], voxels*/,
                           const int* count /*[B * count_stride]*/, int count_stride, int B, int R, int max_n, int top_k,
                           float* travel /*[B,max_n,2]*/, float* cosine /*[B,max_n,2]*/, int* contact /*[B,max_n,2]*/,
                           float* closed /*[B,max_n]*/, void* stream);

/* gnr_volume_objects_fwd: the objects of B volumes [B,R,R,R] -- connected-component labelling of their solid voxels, per component
 * its size, box and coordinate sums, and a copy of the volume with the small components set to free.  What the reference asks its
 * simulator (`while sim.num_objects > 0`, src/gd/experiments/clutter_removal.py:92), answered from the volume.  No reference
 * counterpart; tests/objects_reference.py is the same statement over scipy.ndimage.label and the call produces its bits.  Nothing is
 * floating-point beyond the threshold compare.
 *   lattice    voxel (i,j,k) of scene b sits at ((b*R + i)*R + j)*R + k; k is the world z of the plan's frame, as in gnr_tsdf_*.
 *   solid      lower < (double)v && (double)v < level && k >= z_min, v the voxel's value: a NaN is not solid.
 *   labels     a voxel that is not solid gets 0.  Two solid voxels of one scene are neighbours when their index difference
 *              (di, dj, dk), each in -1..1 and not all 0, has at most 1 (connectivity 6), 2 (18) or 3 (26) non-zero components:
 *              scipy's generate_binary_structure(3, 1 | 2 | 3).  Scenes never join, and neither do the ends of two rows (the
 *              neighbours of a voxel at a face of the lattice are those inside).  A component's label is 1 + the number of components
 *              of its scene whose smallest linear index is smaller: ndimage.label's numbering.  count[b] is the number of components,
 *              the true number even when it exceeds max_objects; the labels are always complete and do not depend on max_objects.
 *   statistics every call first writes rows 0 .. max_objects-1: voxels 0, bbox (R,R,R,-1,-1,-1), sums 0; then, for the labels
 *              1 .. min(count, max_objects), at row label-1: voxels = the component's voxels, bbox = the smallest and the largest i, j, k
 *              (inclusive), sums = the sums of its voxels' i, j and k.  Integer atomics only: any order gives the same bits.
 *   cleaned    (when not NULL) free_value at every voxel of a component with fewer than min_voxels voxels -- of every component,
 *              also those beyond max_objects --, vol's value elsewhere.
 *   workspace  at least gnr_volume_objects_workspace_bytes(B, R) (0 for a B or R outside the limits).  Its first int is the status
 *              word of the call, valid once the stream has run it: 0, or GNR_OBJECTS_STATUS_BOUND when a loop of the labelling ran into
 *              its bound (R^3 links of a chain, R^3 retries of a union; it never spins on) -- the results are then not to be used.
 *              Everything a call reads from its workspace it has written in that call; nothing is kept between calls.
 * 1 <= B <= 65535, 2 <= R <= 256; connectivity 6, 18 or 26; max_objects >= 1; 0 <= z_min <= R; level finite; lower not a NaN;
 * free_value finite.  Asynchronous on `stream`, no allocation, no synchronisation, no float atomics (it can be captured in a graph and
 * replayed); a refused call has launched nothing.                                                                              */
#define GNR_OBJECTS_STATUS_BOUND 1
typedef struct GnrObjectsParams {
    double level;        /* solid: lower < (double)v && (double)v < level; a NaN is not solid.  0.0 for the network's tsdf      */
    double lower;        /* -inf: none.  (-1 keeps out a label volume's "unknown")                                             */
    int    z_min;        /* voxels with k < z_min are not solid (cuts the table slab, on which every object stands); 0: none   */
    int    connectivity; /* 6, 18 or 26: scipy's generate_binary_structure(3, 1 | 2 | 3)                                       */
    int    max_objects;  /* rows of the statistics                                                                             */
    int    min_voxels;   /* for `cleaned`: components with fewer voxels become free_value; <= 1: nothing is removed            */
    float  free_value;   /* 1.0f, the volume's upper clip                                                                      */
} GnrObjectsParams;
size_t gnr_volume_objects_workspace_bytes(int B, int R);
int gnr_volume_objects_fwd(const GnrObjectsParams* params, const float* vol /*[B,R,R,R]*/, int B, int R, int* labels /*[B,R,R,R]*/,
                           int* count /*[B]*/, int* voxels /*[B,max_objects]*/,
                           int* bbox /*[B,max_objects,6]: lo i,j,k, hi i,j,k (inclusive)*/,
                           unsigned long long* sums /*[B,max_objects,3]: sum of i, j, k*/, float* cleaned /*[B,R,R,R] or NULL*/,
                           void* workspace, size_t workspace_bytes, void* stream);

/* gnr_grasp_objects_fwd: which object each ranked grasp would close on -- the samples of the closing region between the pads of
 * gnr_hand_clearance_fwd's hand vote for the label (gnr_volume_objects_fwd's) at their nearest voxel.  The frame, `width`, `pose`,
 * `position` and `rows` are gnr_hand_clearance_fwd's, word for word, as is cell = spacing * scale; finger_width, tail_length and approach
 * are checked and not used.  tests/objects_reference.py is the same statement in numpy and the call produces its bits.
 *   samples    gnr_hand_clearance_fwd's `samples` rule applied to one box, as (lo, extent): x (-0.5 h, h), y (-hw, w), z (0, d); no
 *              approach continuation (m = 0).
 *   votes      a sample with a component outside [0, R-1] (or not a number) is skipped.  The others vote for the label at voxel
 *              ((int)floor(p_x + 0.5), (int)floor(p_y + 0.5), (int)floor(p_z + 0.5)); label 0 (and anything below) casts no vote.
 *   result     inside = the samples taken;  distinct = the number of different labels voted for;  object = the label with the most
 *              votes, of several the smallest, 0 when there is none;  votes = that label's votes.  Integers throughout, any order.
 * The limits of gnr_hand_clearance_fwd, refused with its texts; n_x n_y n_z of a grasp whose width is R voxels must be at most
 * GNR_HAND_MAX_SAMPLES.  Every loop is bounded by the parameters (one pass over the samples per different label, at most as many
 * passes as samples).  Asynchronous on `stream`, no atomics, no workspace, no allocation, no synchronisation (it can be captured in
 * a graph); a refused call has launched nothing.                                                                               */
int gnr_grasp_objects_fwd(const GnrHandParams* hand, const int* labels /*[B,R,R,R]*/, const double* pos /*[B,max_n,3]*/,
                          const float* quat /*[B,max_n,4]*/, const float* width /*[B,max_n], voxels*/, const int* count /*[B * count_stride]*/,
                          int count_stride, int B, int R, int max_n, int top_k, int* object /*[B,max_n]*/, int* votes /*[B,max_n]*/,
                          int* distinct /*[B,max_n]*/, int* inside /*[B,max_n]*/, void* stream);

/* gnr_volume_distance_fwd: the distance field of B volumes [B,R,R,R] -- the exact Euclidean distance transform of their solid mask:
 * per voxel the squared distance to the nearest solid voxel and that voxel, the same to the nearest free voxel, the signed metric
 * field made of the two, and the object (gnr_volume_objects_fwd's label) the nearest solid voxel belongs to.  The volume itself is a
 * truncated field, metric only within a few voxels of a surface; this one is metric everywhere, and every operator that takes a
 * volume (gnr_hand_clearance_fwd above all: by how much the hand misses) takes `esdf` as it is.  No reference counterpart;
 * tests/distance_reference.py is the same statement over scipy.ndimage.distance_transform_edt and the call produces its bits.
 *   lattice    gnr_volume_objects_fwd's: voxel (i,j,k) of scene b sits at ((b*R + i)*R + j)*R + k.
 *   solid      gnr_volume_objects_fwd's rule: lower < (double)v && (double)v < level && k >= z_min; a NaN is not solid.  Every
 *              other voxel is free.
 *   d2_solid   min over the solid voxels (i',j',k') of the SAME scene of (i-i')^2 + (j-j')^2 + (k-k')^2, an integer: 0 at a solid
 *              voxel.  A scene without a solid voxel: 3 R R everywhere (above every real value, 3 (R-1)^2).
 *   nearest_solid  the voxel that attains it, as i' R R + j' R + k' inside its scene; of several the one with the smallest such
 *              index.  A scene without a solid voxel: -1.
 *   d2_free, nearest_free  (both or neither) the same over the free voxels.
 *   esdf       (when not NULL; the free pair is then computed whether it is returned or not) in float64, single correctly rounded
 *              operations in this order:  t = sqrt((double)d2);  t = t - surface_offset;  t = t * scale;  with d2 = d2_solid at a
 *              free voxel, and d2 = d2_free and t = -t at a solid one;  esdf = (float)t.  With surface_offset = 0.5 the surface lies
 *              halfway between a solid voxel and its free neighbour, which read -0.5 and +0.5 voxels.
 *   nearest_label  (when not NULL; needs labels [B,R,R,R], gnr_volume_objects_fwd's) labels[b, nearest_solid], 0 where
 *              nearest_solid is -1.  0 also when the nearest solid voxel carries no label (a table slab the labelling cut by z_min).
 *   workspace  at least gnr_volume_distance_workspace_bytes(B, R) (0 for a B or R outside the limits).  Everything a call reads
 *              from it it has written in that call; nothing is kept between calls.
 * Three line passes (along k, j, i), each min over x' of g[x'] + (x - x')^2 with the smaller x' winning a tie, which leaves the
 * smallest linear index among the nearest voxels.  Every output is fully written.  1 <= B <= 65535, 2 <= R <= 256; 0 <= z_min <= R;
 * level finite; lower not a NaN; scale finite and > 0; surface_offset finite and >= 0; these, a null required pointer, nearest_label
 * without labels and one of the free pair without the other are refused with GNR_ERR_ARG, a workspace too small with
 * GNR_ERR_WORKSPACE.  Asynchronous on `stream`, no atomics, no allocation, no synchronisation, every loop bounded by R (it can be
 * captured in a graph and replayed); a refused call has launched nothing.                                                       */
typedef struct GnrDistanceParams {
    double level;           /* solid: lower < (double)v && (double)v < level; a NaN is not solid.  0.0 for the network's tsdf   */
    double lower;           /* -inf: none                                                                                       */
    double scale;           /* metres per voxel                                                                                 */
    double surface_offset;  /* voxels taken off every distance: 0.5 puts the surface between a solid voxel and its free neighbour */
    int    z_min;           /* voxels with k < z_min are not solid; 0: none                                                     */
} GnrDistanceParams;
size_t gnr_volume_distance_workspace_bytes(int B, int R);
int gnr_volume_distance_fwd(const GnrDistanceParams* params, const float* vol /*[B,R,R,R]*/, const int* labels /*[B,R,R,R] or NULL*/,
                            int B, int R, int* d2_solid /*[B,R,R,R]*/, int* nearest_solid /*[B,R,R,R]*/, int* d2_free /*[B,R,R,R] or NULL*/,
                            int* nearest_free /*[B,R,R,R] or NULL*/, float* esdf /*[B,R,R,R] or NULL*/,
                            int* nearest_label /*[B,R,R,R] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* gnr_volume_parts_fwd: the parts of B integer height fields [B,R,R,R] -- their solid voxels split at the necks: a watershed by
 * steepest ascent, neighbouring basins joined where the pass between them is no neck.  gnr_volume_objects_fwd knows solid voxels and
 * nothing of shapes: objects that touch are one component.  With gnr_volume_distance_fwd's d2_free as the height -- per solid voxel the
 * squared radius of the largest ball around it that stays inside the solid -- two convex things that touch are two hills joined over
 * a low pass, and this call cuts there.  Numbering, statistics rows and calling conventions are gnr_volume_objects_fwd's, so
 * gnr_grasp_objects_fwd takes the labels as they are.  No reference counterpart; tests/parts_reference.py is the same statement in
 * numpy and the call produces its bits.  Nothing is floating-point beyond the one multiply and compare of the neck test.
 *   lattice    gnr_volume_objects_fwd's: voxel (i,j,k) of scene b sits at ((b*R + i)*R + j)*R + k; an index below is that of a voxel
 *              inside its scene, i R R + j R + k.
 *   solid      height > 0.  d2_free is > 0 exactly at the solid voxels of its call, whose solid rule (level, lower, z_min, NaNs) is
 *              not restated here.  Any int32 field is accepted.
 *   neighbours gnr_volume_objects_fwd's, under connectivity 6, 18 or 26, inside the same scene: rows, planes and scenes do not wrap.
 *   ascent     up[v] is the voxel of the largest height among the solid voxel v and its solid neighbours, of several with that
 *              height the one of the smallest index; v takes part in both comparisons.  A voxel with up[v] == v is a summit.
 *              Following up from any solid voxel ends at a summit (every link strictly increases (height, -index)): the voxel's
 *              basin, whose peak is the summit's height.  basins[b] is the number of summits of scene b.
 *   merge      for every pair of neighbouring solid voxels u, w in different basins a, b, with pass = min(height[u], height[w]):
 *              the two basins are joined when min(peak_a, peak_b) <= min_peak, or when
 *                  (double)pass >= (neck * neck) * (double)min(peak_a, peak_b)
 *              -- neck * neck one double multiply, then one double multiply and one compare, the same on host and device.  The
 *              peaks are the basins' own, never those of an already merged set, so the set of joins does not depend on any order.
 *              The parts are the transitive closure of the joins.  neck is a ratio of radii: with heights from d2_free it compares
 *              the half-width of the pass with the inscribed radius of the smaller hill.  neck = 0 joins every pair of adjoining
 *              basins: the labels are then gnr_volume_objects_fwd's of the same solid voxels and connectivity.  On a plateau (all
 *              heights equal) every summit merges for every neck <= 1, which is why neck > 1 is refused.
 *   labels     a voxel that is not solid gets 0.  A part's label is 1 + the number of parts of its scene whose smallest index is
 *              smaller: ndimage.label's numbering.  count[b] is the number of parts, the true number even when it exceeds max_parts;
 *              the labels are always complete and do not depend on max_parts.
 *   statistics gnr_volume_objects_fwd's rows and empty values, and two columns more: every call first writes rows 0 .. max_parts-1:
 *              voxels 0, bbox (R,R,R,-1,-1,-1), sums 0, peak 0, peak_voxel -1; then, for the labels 1 .. min(count, max_parts), at
 *              row label-1: voxels, bbox and sums of the part's voxels, peak = the largest height in the part, peak_voxel = the smallest
 *              index in the part that has that height.  Integer atomics only: any order gives the same bits.
 *   workspace  at least gnr_volume_parts_workspace_bytes(B, R) (0 for a B or R outside the limits).  Its first int is the status word
 *              of the call, valid once the stream has run it: 0, or GNR_PARTS_STATUS_BOUND when a loop ran into its bound (R^3 links
 *              of a walk or a chain, R^3 retries of a union; it never spins on) -- the results are then not to be used.  Everything a
 *              call reads from its workspace it has written in that call; nothing is kept between calls.
 * 1 <= B <= 65535, 2 <= R <= 256 (GNR_ERR_SHAPE); connectivity 6, 18 or 26 (GNR_ERR_ARG); max_parts >= 1 (GNR_ERR_SHAPE);
 * min_peak >= 0; neck finite and in [0, 1] (GNR_ERR_ARG); a null pointer (GNR_ERR_ARG); a workspace too small (GNR_ERR_WORKSPACE).
 * Asynchronous on `stream`, no allocation, no synchronisation, no float atomics (it can be captured in a graph and replayed); a
 * refused call has launched nothing.
 * What it cannot separate: two boxes face to face without a gap are one box to any rule that sees the solid voxels alone; a part
 * whose own waist is narrower than `neck` times its smaller bulge is cut in two.  neck = 0.8 separates the synthetic touching shapes
 * of tests/test_volume_parts.py; it has not been run on a network's volume.                                                       */
#define GNR_PARTS_STATUS_BOUND 1
typedef struct GnrPartsParams {
    double neck;         /* in [0, 1]: a pass is a neck when its height is below neck^2 times the smaller of the two peaks; 0: none    */
    int    connectivity; /* 6, 18 or 26: scipy's generate_binary_structure(3, 1 | 2 | 3)                                       */
    int    max_parts;    /* rows of the statistics                                                                             */
    int    min_peak;     /* a basin whose peak is at most this joins every basin it adjoins (ripples of a rough surface); 0: none  */
} GnrPartsParams;
size_t gnr_volume_parts_workspace_bytes(int B, int R);
int gnr_volume_parts_fwd(const GnrPartsParams* params, const int* height /*[B,R,R,R]*/, int B, int R, int* labels /*[B,R,R,R]*/,
                         int* count /*[B]*/, int* basins /*[B]*/, int* voxels /*[B,max_parts]*/,
                         int* bbox /*[B,max_parts,6]: lo i,j,k, hi i,j,k (inclusive)*/,
                         unsigned long long* sums /*[B,max_parts,3]: sum of i, j, k*/, int* peak /*[B,max_parts]*/,
                         int* peak_voxel /*[B,max_parts]*/, void* workspace, size_t workspace_bytes, void* stream);

/* gnr_grasp_retreat_fwd: whether the part each ranked grasp holds comes out of the pile -- the fourth step of execute_grasp
 * (gd/simulation.py:369-422): after the fingers closed, the hand moves `retreat` metres back along its own z, or, when the approach
 * is more than 60 degrees off straight down, lifts that far along world +z (:378-386, 406), and only then asks check_success.  The
 * voxels of the held part (gnr_volume_parts_fwd's or gnr_volume_objects_fwd's label, gnr_grasp_objects_fwd's `object`) are moved
 * along that line by integer offsets, and every step counts those that land inside another part.  No reference counterpart;
 * tests/retreat_reference.py is the same statement in numpy and the call produces its bits.  quat converts to float64 before the
 * first operation; all arithmetic is float64, single correctly rounded operations in the order written, never contracted;
 * everything else is integers.
 *   lattice    gnr_volume_objects_fwd's: voxel (i,j,k) of scene b sits at ((b*R + i)*R + j)*R + k; axis 2 (k) is the world's z, the
 *              axis the solid rule's z_min cuts.
 *   steps      T = retreat / scale (voxels);  K = (int)fmax(1, ceil(T / step));  sl = T / (double)K.  K depends on the parameters
 *              alone and must be at most GNR_RETREAT_MAX_STEPS.
 *   pose       M is gnr_hand_clearance_fwd's matrix of (double)quat[b,r], word for word (the division by fmax(norm, 1e-12)
 *              included);  u_a = -M[a][2] for a = 0, 1, 2.  If any u_a is not a number the row moves nothing: every integer output
 *              of the row is 0 and travel = (float)(T * scale).
 *   direction  side = (-M[2][2] < side_cos) ? 1 : 0;  with side set, u = (0, 0, 1).
 *   moving     L = held[b,r].  L < 1 or L > max_parts: no voxel moves.  Otherwise lo_a = max(bbox[b,L-1,a], 0), hi_a =
 *              min(bbox[b,L-1,3+a], R-1), and the moving voxels are the voxels v of that box (none when some lo_a > hi_a) with
 *              labels[b,v] == L.  moved = their number.  A box wider than the part gives the part's own result.
 *   step k     for k = 1 .. K:  o_a = rint(u_a * ((double)k * sl)) -- to nearest, ties to even; an integer, not an int32: a
 *              |o_a| >= R moves every voxel out --;  t = v + o.  A t with a component outside [0, R-1] has left the workspace and
 *              hits nothing: it never wraps into a neighbouring row, plane or scene.  Otherwise v hits when labels[b,t] is
 *              neither 0 nor L (labels are any int32).  hits_k = the number of moving voxels that hit.
 *   result     overlap = max_k hits_k;  blocked_step = the smallest k with hits_k > tolerance, 0 when there is none;  blocker =
 *              labels[b, v* + o] at k = blocked_step, v* the moving voxel of the smallest index i R R + j R + k that hits there, 0
 *              when not blocked;  travel = (float)(((double)(blocked_step - 1) * sl) * scale) when blocked, else
 *              (float)(T * scale): metres moved before the first blocked step;  side as above.
 *   rows       gnr_hand_clearance_fwd's: r < min(count[b * count_stride], top_k > 0 ? top_k : max_n, max_n); the other rows are
 *              left untouched.
 * 1 <= B <= 65535, 2 <= R <= 256, max_n >= 1 (GNR_ERR_SHAPE); count_stride >= 1, top_k >= 0; retreat, step and scale finite and
 * > 0; side_cos finite; tolerance >= 0 (GNR_ERR_ARG); max_parts >= 1 (GNR_ERR_SHAPE); K within the cap, a null pointer
 * (GNR_ERR_ARG).  Every loop is bounded by the parameters and R: no content of bbox, held, quat or count ends one later or moves
 * an access out of the scene's lattice.  Asynchronous on `stream`, no global-memory atomics, no workspace, no allocation, no
 * synchronisation (it can be captured in a graph); a refused call has launched nothing.
 * What it does not answer: the closed hand's own sweep on the lift, any rotation of the part, parts that would be pushed aside
 * rather than block.  Which parts rest on the held one, and which lose their footing once it is gone, is gnr_part_support_fwd's
 * answer; what the pile then does -- anything that slides, tips or settles (remove_and_wait) -- is nobody's.                   */
#define GNR_RETREAT_MAX_STEPS 1024
typedef struct GnrRetreatParams {
    double retreat;    /* metres the hand moves away: 0.1 (simulation.py:382,385)                                              */
    double step;       /* voxels between tested positions at most: 0.5                                                         */
    double side_cos;   /* a grasp whose approach has -a_z < side_cos lifts along world +z: 0.5 = cos(pi/3)                     */
    double scale;      /* metres per voxel                                                                                     */
    int    tolerance;  /* a step is blocked when MORE than this many moving voxels are inside other parts: 0                   */
    int    max_parts;  /* rows of bbox                                                                                         */
} GnrRetreatParams;
int gnr_grasp_retreat_fwd(const GnrRetreatParams* params, const int* labels /*[B,R,R,R]*/, const int* bbox /*[B,max_parts,6]*/,
                          const int* held /*[B,max_n]*/, const float* quat /*[B,max_n,4]*/, const int* count /*[B * count_stride]*/,
                          int count_stride, int B, int R, int max_n, int top_k, int* blocked_step /*[B,max_n]*/, int* blocker /*[B,max_n]*/,
                          int* overlap /*[B,max_n]*/, int* moved /*[B,max_n]*/, int* side /*[B,max_n]*/, float* travel /*[B,max_n]*/,
                          void* stream);

/* gnr_part_contacts_fwd, gnr_part_support_fwd: the support of the parts -- where two labels of a label volume touch, which of the two
 * lies on the other there, and the graph that follows: on whom a part rests, what it carries, which parts lose every footing when it
 * is taken, in which order a pile comes apart without anything falling, what hangs in the air.  gnr_grasp_retreat_fwd tests one line
 * for one part; this looks at pairs of labels.  The reference leaves the question to physics (remove_and_wait, gd/simulation.py;
 * `while sim.num_objects > 0`, clutter_removal.py:92).  No reference counterpart; tests/support_reference.py is the same statement in
 * numpy and the calls produce its bits.  Integers throughout, but for the one double multiply and compare of the lean test.
 *   lattice    gnr_volume_objects_fwd's: voxel (i,j,k) of scene b sits at ((b*R + i)*R + j)*R + k; axis 2 (k) is the world's z.
 *   labels     any int32 volume (gnr_volume_parts_fwd's or gnr_volume_objects_fwd's `labels`).  A label < 1 is no part.  P =
 *              max_parts is the number of rows of every table: part a is row a-1.
 *   neighbours gnr_volume_objects_fwd's, under connectivity 6, 18 or 26, inside the same scene: rows, planes and scenes do not wrap.
 * gnr_part_contacts_fwd: labels -> tables.
 *   pairs      for every ORDERED pair of neighbouring voxels (u, w) of scene s, with a = labels[u], b = labels[w], a >= 1, b >= 1
 *              and a != b:  if a <= P and b <= P, touch[s,a-1,b-1] += 1, and, when k_w > k_u (b's voxel is the higher one: b lies on
 *              a there), over[s,a-1,b-1] += 1;  otherwise dropped[s] += 1.  touch is symmetric by construction.  pairs[s,a-1,b-1,0] =
 *              touch, pairs[s,a-1,b-1,1] = over.
 *   floor      floor[s,a-1] = the number of voxels with label a in 1..P and k == z_min: with z_min cutting the table slab these
 *              voxels stand on the table.  z_min == R gives none.
 *   Every element of pairs, floor and dropped is written by every call (a fill kernel, then integer atomics: any order gives the
 *   same bits).
 * gnr_part_support_fwd: tables -> graph.  Per scene n = min(max(count[s], 0), P); the parts are the labels 1..n.
 *   rests      with N = touch[a,c] and D = over[a,c] - over[c,a]:  rests(c, a), "c rests on a", holds when a != c, N >= min_contact,
 *              D > 0 and (double)D >= lean * (double)N -- one double multiply and one compare.  Antisymmetric in D: never both ways.
 *              on_floor(a) = floor[a] >= min_floor.
 *   below[a]   the number of c with rests(a, c): a's footings.      above[a]  the number of c with rests(c, a).
 *   carried[a] the number of parts other than a reachable from a along "rests on a", transitively.
 *   orphans[a] F starts as {a}; a round adds every c that is not in F, is not on_floor, has below[c] >= 1 and has all its footings in
 *              F; rounds repeat until nothing changes (at most n do).  orphans[a] = |F| - 1: the parts that lose every footing when
 *              a is taken.
 *   layer[a]   0 when above[a] == 0, otherwise 1 + the largest layer of the parts resting on a, assigned only once all of those are
 *              assigned (at most n rounds); a part still unassigned then gets -1: the relation has a cycle above it.  Any int32
 *              label volume can make one; the parts' labels should not.  Ascending (layer, label) is an order in which nothing
 *              taken has anything resting on it.
 *   grounded[a]  1 when on_floor(a) or some footing of a is grounded (a fixed point, at most n rounds), otherwise 0.
 *   rests_on   (when not NULL) rests_on[s,c-1,a-1] = rests(c, a) as 0 / 1, for c, a in 1..n; 0 elsewhere.
 *   Rows n .. P-1 of every output are written as the empty values: the counts 0, layer -1, grounded 0.
 * Limits, in the order they are refused (a null `params` comes first: GNR_ERR_ARG "null pointer"): 1 <= B <= 65535 and, for the
 * contacts, 2 <= R <= 256 (GNR_ERR_SHAPE); 1 <= max_parts <= GNR_SUPPORT_MAX_PARTS (GNR_ERR_SHAPE: the table is dense, 256 rows are
 * 512 KB per scene; a heap of more parts is not what this answers, and `dropped` says when labels went beyond the rows); connectivity
 * 6, 18 or 26; 0 <= z_min <= R; min_contact >= 1; min_floor >= 1; lean finite and in [0, 1]; a null required pointer (GNR_ERR_ARG).
 * The support call has no R.  Both calls: asynchronous on `stream`, no workspace, no allocation, no synchronisation, no float
 * atomics, every loop bounded by R, P or 64 (they can be captured in a graph and replayed); a refused call has launched nothing and
 * written nothing.
 * What it does not answer: any dynamics -- nothing slides, tips or settles --, contact points and normals in metres, whether a
 * part's centre of mass lies over its footings.  lean = 0.25 lies between the 0.0 of every side contact and the 0.83 .. 1.0 of every
 * resting contact of the synthetic piles of tests/test_part_support.py; it has not been run on a network's volume.                */
#define GNR_SUPPORT_MAX_PARTS 256
typedef struct GnrContactsParams {
    int connectivity;  /* 6, 18 or 26: the parts' own                                                                          */
    int max_parts;     /* P: rows of the tables, 1 .. GNR_SUPPORT_MAX_PARTS                                                    */
    int z_min;         /* the plane whose voxels stand on the table: the solid rule's z_min; R: none                           */
} GnrContactsParams;
int gnr_part_contacts_fwd(const GnrContactsParams* params, const int* labels /*[B,R,R,R]*/, int B, int R, int* pairs /*[B,P,P,2]*/,
                          int* floor /*[B,P]*/, int* dropped /*[B]*/, void* stream);
typedef struct GnrSupportParams {
    double lean;         /* in [0, 1]: c rests on a when over[a,c] - over[c,a] >= lean * touch[a,c]: 0.25                      */
    int    max_parts;    /* P: rows of the tables and of every output                                                          */
    int    min_contact;  /* fewer touching voxel pairs are no contact: 1                                                       */
    int    min_floor;    /* a part with at least this many voxels in the floor plane stands on the table: 1                    */
} GnrSupportParams;
int gnr_part_support_fwd(const GnrSupportParams* params, const int* pairs /*[B,P,P,2]*/, const int* floor /*[B,P]*/,
                         const int* count /*[B]*/, int B, int* below /*[B,P]*/, int* above /*[B,P]*/, int* carried /*[B,P]*/,
                         int* orphans /*[B,P]*/, int* layer /*[B,P]*/, int* grounded /*[B,P]*/,
                         unsigned char* rests_on /*[B,P,P] or NULL*/, void* stream);

/* gnr_part_feet_fwd, gnr_part_balance_fwd: the balance of the parts -- on which of its voxels a part stands, whether its centre of mass
 * lies over them, by how much, and what tips over, and falls, when a part is taken.  gnr_part_support_fwd's orphans are the parts that
 * lose EVERY footing; the commoner failure of a pile is a part that keeps one footing and tips over it (a plank across two pillars,
 * one pillar taken).  The reference leaves the question to physics (remove_and_wait, gd/simulation.py).  No reference counterpart;
 * tests/balance_reference.py is the same statement in numpy and the calls produce its bits.  Integers throughout, but for one double
 * multiply and one double divide per direction of a margin, never contracted.
 *   lattice, labels, neighbours   gnr_part_contacts_fwd's: k is up; P = max_parts rows, part c is row c-1; n = min(max(count[s], 0), P),
 *              the parts are the labels 1..n.
 *   rests_on   [B,P,P] bytes, gnr_part_support_fwd's or any: [c-1,a-1] != 0 reads "c rests on a".
 * gnr_part_feet_fwd: labels and relation -> tables.
 *   slots      Part c has GNR_BALANCE_SLOTS = 8 foot slots.  Slot 0 is the floor plane k == z_min.  The footings of c <= n are the a
 *              with rests_on[c-1,a-1] != 0, a <= n, a != c; they take the slots 1, 2, .. in ascending label order, and from the
 *              seventh on they share slot 7.  slots[s,c-1,a-1] (uint8) is the slot of footing a, 0 where a is no footing of c; the rows
 *              of c > n hold 0.  crowded[s,c-1] = 1 when slot 7 holds two or more footings (eight footings or more), else 0.
 *   feet       A voxel u with label c, 1 <= c <= P, is a foot in slot 0 when k_u == z_min, and a foot in slot t >= 1 when some
 *              neighbour w with k_w < k_u carries a label a with 1 <= a <= P, a != c and slots[c-1,a-1] == t.  A voxel counts once per
 *              slot and may be in several.  feet[s,c-1,t] (int32) is the number of foot voxels of slot t.  z_min == R: no slot 0.
 *   reach      reach[s,c-1,t,q] (int32) = the largest dx_q * i + dy_q * j over the foot voxels of slot t, INT32_MIN where there are
 *              none.  The GNR_BALANCE_DIRECTIONS = 16 directions (dx, dy) are (1,0) (2,1) (1,1) (1,2) (0,1) (-1,2) (-1,1) (-2,1), then
 *              their negatives in the same order.
 *   moments    moments[s,c-1,:] (int64) = n_c, sum i, sum j, sum k, sum i^2, sum j^2, sum k^2, sum i j, sum i k, sum j k over the voxels
 *              with label c.  Labels outside 1..P are ignored (gnr_part_contacts_fwd's `dropped` reports them).
 *   Every element of moments, slots, feet, reach and crowded is written by every call (a fill kernel, then integer atomics: any
 *   order gives the same bits).
 * gnr_part_balance_fwd: tables -> balance.
 *   balance    of a mass (m, Si, Sj) over a set of slots of part c.  A slot is usable when feet[c-1,t] >= 1, slot 0 when feet[c-1,0]
 *              >= min_floor.  r_q = the largest reach[c-1,t,q] over the usable slots of the set; H_q = 2 r_q + |dx_q| + |dy_q| -- the
 *              support function, doubled, of the hull of the foot voxels' unit squares; num_q = m * H_q - 2 * (dx_q * Si + dy_q * Sj)
 *              in int64.  Balanced: every num_q >= 0.  margin = the least (double)num_q / ((double)(2 m) * len_q), in voxels, with
 *              len_q = 1, sqrt 2 or sqrt 5 as the nearest double: one multiply, then one divide.  With no usable slot in the set, or
 *              with m < 1, the mass is not balanced and the margin is -inf.
 *   balanced[c], margin[c]   for c <= n: the balance of c's own mass (moments[c-1,0..2]) over all its slots.
 *   tips       tips[s,c-1,a-1] = 1 for c, a <= n, c != a, with rests_on[c-1,a-1] != 0, when c's own mass is not balanced over its
 *              slots other than slots[c-1,a-1] (read & 7); 0 elsewhere.  When a shares the crowded slot 7 the whole slot goes: on
 *              the careful side.
 *   unsettles[a]  the number of c with tips[c-1,a-1].
 *   falls[a]   the number of parts other than a among those c and everything they carry (gnr_part_support_fwd's closure of "rests
 *              on", over this call's rests_on).  falls >= orphans, element by element, when rests_on, count, z_min and min_floor are
 *              the support's own.
 *   Rows n .. P-1 hold balanced 0, margin -inf, unsettles 0, falls 0.
 * Limits, in the order they are refused (a null `params` comes first: GNR_ERR_ARG "null pointer"): 1 <= B <= 65535 and, for the
 * feet, 2 <= R <= 256 (GNR_ERR_SHAPE); 1 <= max_parts <= GNR_BALANCE_MAX_PARTS (GNR_ERR_SHAPE); connectivity 6, 18 or 26; 0 <= z_min
 * <= R; min_floor >= 1; a null required pointer (GNR_ERR_ARG; `tips` may be NULL).  The balance call has no R; its int64 products are
 * exact on the tables of the feet call (m <= 2^24, coordinates <= 255) and wrap on others.  Both calls: asynchronous on `stream`, no
 * workspace, no allocation, no synchronisation, no float atomics, every loop bounded by P, 64, 16 or 8 (they can be captured in a
 * graph and replayed); a refused call has launched nothing and written nothing.
 * What it does not answer.  It is the statics of each part's own mass: what a part carries does not shift its balance point, and
 * nothing slides or rotates.  A part on a single floor voxel reads a margin of 0.5 (voxelised balls do).  Under connectivity 18 or 26
 * a foot voxel may overhang its footing by one diagonal; connectivity 6 gives the strict footprint.  There is no threshold of its
 * own: the rule is integer geometry plus the support's min_floor.  It has not been run on a network's volume.                      */
#define GNR_BALANCE_MAX_PARTS 256
#define GNR_BALANCE_SLOTS 8
#define GNR_BALANCE_DIRECTIONS 16
typedef struct GnrFeetParams {
    int connectivity;  /* 6, 18 or 26: the parts' own                                                                          */
    int max_parts;     /* P: rows of the tables, 1 .. GNR_BALANCE_MAX_PARTS                                                    */
    int z_min;         /* the floor plane: the solid rule's z_min; R: none                                                     */
} GnrFeetParams;
int gnr_part_feet_fwd(const GnrFeetParams* params, const int* labels /*[B,R,R,R]*/, const unsigned char* rests_on /*[B,P,P]*/,
                      const int* count /*[B]*/, int B, int R, long long* moments /*[B,P,10]*/, unsigned char* slots /*[B,P,P]*/,
                      int* feet /*[B,P,8]*/, int* reach /*[B,P,8,16]*/, int* crowded /*[B,P]*/, void* stream);
typedef struct GnrBalanceParams {
    int max_parts;     /* P: rows of the tables and of every output                                                            */
    int min_floor;     /* slot 0 is usable with at least this many voxels in the floor plane: the support's, 1                 */
} GnrBalanceParams;
int gnr_part_balance_fwd(const GnrBalanceParams* params, const long long* moments /*[B,P,10]*/, const int* feet /*[B,P,8]*/,
                         const int* reach /*[B,P,8,16]*/, const unsigned char* slots /*[B,P,P]*/, const unsigned char* rests_on /*[B,P,P]*/,
                         const int* count /*[B]*/, int B, int* balanced /*[B,P]*/, double* margin /*[B,P]*/, int* unsettles /*[B,P]*/,
                         int* falls /*[B,P]*/, unsigned char* tips /*[B,P,P] or NULL*/, void* stream);

/* gnr_part_overlap_fwd, gnr_part_track_fwd: parts across two plans -- which part of the label volume of plan t is which part of the
 * label volume of plan t+1, and what became of every part: it stayed, it moved, it is gone, it was absorbed into another; a part of
 * the second volume is the same as before, new, or a fragment.  gnr_volume_parts_fwd numbers each volume on its own, in voxel order,
 * so taking one ball renumbers every part behind it; the labels of two plans say nothing about each other until their voxels are
 * compared.  The reference reads the answer off its simulator (check_success, remove_body, remove_and_wait: clutter_removal.py:92-150,
 * gd/simulation.py); on the real-robot route the next plan's volume is the only witness of a take.  No reference counterpart;
 * tests/track_reference.py is the same statement in numpy and the calls produce its bits.  Integers throughout, but for two kinds of
 * double multiply and compare (share, stay), never contracted.
 *   before, after   any int32 label volumes [B,R,R,R] on the same lattice (gnr_volume_objects_fwd's), 2 <= R <= 256.  A label < 1 is
 *              no part.  P = max_parts.  index(l) = l for 1 <= l <= P, 0 for l < 1, and *beyond* for l > P.
 * gnr_part_overlap_fwd: volumes -> table.
 *   table      [B,P+1,P+1] int32: table[s,i,j] counts the voxels of scene s with index(before) = i and index(after) = j, neither
 *              beyond, (i,j) != (0,0).  table[s,0,0] is written as 0: voxels free in both are not counted.  Row 0 is "was free",
 *              column 0 is "is free now".
 *   beyond     [B] int32: the voxels where either label is > P.
 *   Every element of both is written by every call (a fill kernel, then integer atomics: any order gives the same bits).
 * gnr_part_track_fwd: table and counts -> fates.  Per scene nb = min(max(count_before[s], 0), P) and na likewise from count_after;
 * the old parts are the labels 1..nb, the new parts 1..na; only rows 0..nb and columns 0..na of the table are read.
 *   size_before[a] = sum over j = 0..na of table[a,j];  size_after[b] = sum over i = 0..nb of table[i,b]  (int32 sums: a table of
 *              gnr_part_overlap_fwd holds at most R^3 <= 2^24 in all; on any other table the sums wrap as unsigned adds do).
 *   heir[a]    the b in 1..na with the largest table[a,b], ties to the smallest b; kept only if that count t >= 1 and
 *              (double)t >= share * (double)size_before[a]; otherwise 0.  Where most of a's voxels are now.
 *   source[b]  the a in 1..nb with the largest table[a,b], ties to the smallest a; kept only if t >= 1 and
 *              (double)t >= share * (double)size_after[b]; otherwise 0.  What b is mostly made of.
 *   a and b are the same part when heir[a] == b and source[b] == a.
 *   per old part, [B,P] int32, part a in row a-1:
 *     heir       as above                                  shared     the largest table[a,1..na], even below share; 0 when na == 0
 *     size_before                                          vacated    table[a,0]
 *     pieces     the number of b with source[b] == a
 *     fate       0 STAYED  the same part, and (double)t >= stay * (double)(size_before[a] + size_after[b] - t): t over the union
 *                1 MOVED   the same part, below stay
 *                2 GONE    heir == 0
 *                3 MERGED  heir[a] = b != 0 but source[b] != a: it was absorbed into something else
 *     Rows nb .. P-1 hold 0, and fate -1.
 *   per new part, [B,P] int32, part b in row b-1:
 *     source     as above                                  size_after
 *     fresh      table[0,b]                                absorbed   the number of a with heir[a] == b
 *     origin     0 SAME;  1 NEW: source == 0;  2 FRAGMENT: source[b] = a != 0 but heir[a] != b
 *     Rows na .. P-1 hold 0, and origin -1.
 *   summary    [B,8] int32: nb, na, stayed, moved, gone, merged, new, fragments.
 * Limits, in the order they are refused (a null `params` comes first: GNR_ERR_ARG "null pointer"): 1 <= B <= 65535 and, for the
 * overlap, 2 <= R <= 256 (GNR_ERR_SHAPE); 1 <= max_parts <= GNR_TRACK_MAX_PARTS (GNR_ERR_SHAPE: the table is dense, 257 x 257 words
 * are 258 KB per scene, and `beyond` says when labels went beyond the rows); share, then stay, finite and in [0, 1]; a null pointer
 * (GNR_ERR_ARG).  The track call has no R.  Both calls: asynchronous on `stream`, no workspace, no allocation, no synchronisation, no
 * float atomics, every loop bounded by P + 1 or 64 (they can be captured in a graph and replayed); a refused call has launched nothing
 * and written nothing.
 * What it does not answer.  The match is by overlap alone: a part that moved by more than about its own radius shares too few voxels
 * with itself and reads GONE next to a NEW part -- it is not followed; nothing is matched by shape, and nothing turns.  share = 0.5 and
 * stay = 0.6 are policy, not measurement: on synthetic balls of radius 3, 5, 8 voxels a shift of one voxel reads STAYED (overlap over
 * union 0.62, 0.73, 0.83), a shift up to about 0.6 of the radius MOVED, more GONE + NEW (tests/test_part_track.py has the table).
 * Neither has been run on a network's volumes, whose surface noise between two plans nobody has measured; the integer columns shared,
 * size, vacated and fresh let a caller apply thresholds of their own.                                                              */
#define GNR_TRACK_MAX_PARTS 256
#define GNR_TRACK_STAYED 0
#define GNR_TRACK_MOVED 1
#define GNR_TRACK_GONE 2
#define GNR_TRACK_MERGED 3
#define GNR_TRACK_SAME 0
#define GNR_TRACK_NEW 1
#define GNR_TRACK_FRAGMENT 2
typedef struct GnrOverlapParams {
    int max_parts;     /* P: the table has P + 1 rows and columns, 1 .. GNR_TRACK_MAX_PARTS                                    */
} GnrOverlapParams;
int gnr_part_overlap_fwd(const GnrOverlapParams* params, const int* before /*[B,R,R,R]*/, const int* after /*[B,R,R,R]*/, int B, int R,
                         int* table /*[B,P+1,P+1]*/, int* beyond /*[B]*/, void* stream);
typedef struct GnrTrackParams {
    double share;      /* in [0, 1]: an heir / a source holds at least this share of the part's voxels: 0.5                    */
    double stay;       /* in [0, 1]: the same part STAYED when the shared voxels are at least this share of the union: 0.6     */
    int    max_parts;  /* P: the table's, and the rows of every output                                                         */
} GnrTrackParams;
int gnr_part_track_fwd(const GnrTrackParams* params, const int* table /*[B,P+1,P+1]*/, const int* count_before /*[B]*/,
                       const int* count_after /*[B]*/, int B, int* heir /*[B,P]*/, int* shared /*[B,P]*/, int* size_before /*[B,P]*/,
                       int* vacated /*[B,P]*/, int* pieces /*[B,P]*/, int* fate /*[B,P]*/, int* source /*[B,P]*/, int* size_after /*[B,P]*/,
                       int* fresh /*[B,P]*/, int* absorbed /*[B,P]*/, int* origin /*[B,P]*/, int* summary /*[B,8]*/, void* stream);

/* ---- depth route: TSDF fusion of posed depth images (src/gd/perception.py:66-128 over Open3D's UniformTSDFVolume, no colour) ----
 * State per scene: tsdf [R,R,R] and weight [R,R,R], float32, voxel (x,y,z) at x*R*R + y*R + z (the order of volume[0,0,x,y,z]), zero
 * after gnr_tsdf_reset.  gnr_tsdf_integrate fuses V views per scene into it, in the order given, for every voxel:
 *   p = origin + (idx + 0.5) * voxel_size;  pc = R_wc p + t  (poses: world->camera, OpenCV axes);  skip the view if pc.z <= 0
 *   u_f = pc.x * fx / pc.z + cx + 0.5, v_f likewise;  skip unless 1e-4 <= u_f < w - 1e-4 and 1e-4 <= v_f < h - 1e-4;  u = (int)u_f, v = (int)v_f
 *   d = depth[v,u] / depth_scale;  d >= depth_trunc -> d = 0;  skip if d <= 0
 *   sdf = (d - pc.z) * sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1)
 *   if sdf > -sdf_trunc:  t = min(1, sdf / sdf_trunc);  tsdf = (tsdf * weight + t) / (weight + 1);  weight += 1
 * Everything up to t is float64 (single correctly rounded operations in this order, never contracted), t is rounded once to
 * float32, the update is float32: V views in one call and V calls of one view give the same bits, and the result equals the
 * float64 statement of tests/tsdf_reference.py bit for bit.
 *   depth [B,V,h,w] float32 (GNR_DEPTH_F32) or uint16 (GNR_DEPTH_U16);  poses [B,V,3,4];  Ks [B,V,3,3];  origin [B,3]
 *   1 <= B <= 65535, V >= 1, h, w >= 1, 2 <= R <= 256;  voxel_size, sdf_trunc, depth_scale, depth_trunc > 0
 * gnr_tsdf_grid: GNR_TSDF_GRID       out = (tsdf + 1) / 2 where weight != 0 and -0.98 <= tsdf < 0.98, else 0   (get_grid)
 *                GNR_TSDF_SDF_LABEL  out = grid * 2 - 1: the trainer's sdf_gt, -1 = no label   (dataset/database.py:207-209)
 * All three are asynchronous on `stream`, allocate nothing and do not synchronise (they can be captured in a graph); a refused
 * call (GNR_ERR_ARG / GNR_ERR_SHAPE) has launched nothing.                                                               */
#define GNR_DEPTH_F32 0
#define GNR_DEPTH_U16 1
#define GNR_TSDF_GRID 0
#define GNR_TSDF_SDF_LABEL 1
typedef struct GnrTsdfParams {
    int B, V, h, w, R, depth_dtype;            /* GNR_DEPTH_*                                           */
    double voxel_size, sdf_trunc, depth_scale, depth_trunc;
} GnrTsdfParams;
int gnr_tsdf_reset(int B, int R, float* tsdf, float* weight, void* stream);
int gnr_tsdf_integrate(const GnrTsdfParams* params, const void* depth /*[B,V,h,w]*/, const float* poses /*[B,V,3,4]*/,
                       const float* Ks /*[B,V,3,3]*/, const float* origin /*[B,3]*/, float* tsdf, float* weight /*[B,R,R,R] in/out*/,
                       void* stream);
int gnr_tsdf_grid(int B, int R, const float* tsdf, const float* weight, int mode /*GNR_TSDF_GRID | GNR_TSDF_SDF_LABEL*/, float* out /*[B,R,R,R]*/, void* stream);

/* ---- introspection / measurement -------------------------------------------------------*/
/* name of the dominant kernel as it appears in rocprofv3 traces, and the calling thread's last error text (see GNR_ERR_*) */
const char* gnr_dominant_kernel_name(void);
const char* gnr_last_error(void);
/* In-situ timing (process-wide switch, measurement only): between gnr_timing_begin() and gnr_timing_end() every kernel
 * launch of the library is bracketed by a pair of HIP events recorded on ITS launch stream (nothing else is added to the
 * path).  gnr_timing_end() waits for the events and writes one line per label -- "label count total_ms\n", label =
 * "kernel@entry point" (k_chain / k_ray: "k_chain.volume", "k_chain.render", "...train") -- into `report` (NUL-terminated,
 * truncated to report_bytes); returns the number of launches recorded or a negative error code.
 * Event pairs around EVERY launch cost a few microseconds of pipeline bubble each (11 launches per forward step: ~2 % of the
 * step), so a headline measurement brackets its dominant kernel only (gnr_timing_begin_only) and takes the full table in a
 * separate pass.  gnr_chain_timing_begin/end: the same switch for the k_chain launches on volume points, reduced to their
 * average duration. */
int gnr_timing_begin(void);
int gnr_timing_begin_only(const char* label_substring);   /* bracket only the launches whose label contains the substring */
int gnr_timing_end(char* report, size_t report_bytes);
int gnr_chain_timing_begin(void);
int gnr_chain_timing_end(float* avg_ms_out, int* count_out);
/* Time `iters` launches of the dominant kernel alone (volume points of `scene`) with HIP
 * events on `stream`; returns average milliseconds per launch in *ms_out. */
int gnr_time_chain_kernel(const GnrScene* scene, int volume_res, const float* packed_coarse,
                          void* workspace, size_t workspace_bytes, int iters, float* ms_out, void* stream);

/* Test tooling: fill the LDS of every CU with a 32-bit pattern (LDS is not cleared between kernels; a kernel that reads LDS it did
 * not write would compute on it).  tests/test_range_guard.py runs the path after two patterns and asks for identical bits. */
int gnr_debug_fill_lds(unsigned pattern, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNR_H */

# The library's translation units and hipcc flags, in one place (sourced by build.sh, tools/build_variant.sh, tools/text_hash.sh).
# -fno-slp-vectorize: packed f32 VALU (v_pk_fma_f32 / v_pk_mul_f32 from SLP-packed scalar code) costs more than the
# two scalar ops it replaces when it sits between MFMAs (MI355X_MICROARCH.md); measured -1 % on k_chain, -1.2 % per step.
SRC="gnr_kernels.hip gnr_head.hip gnr_post.hip gnr_mesh.hip gnr_raycast.hip gnr_surface_color.hip gnr_hand.hip gnr_objects.hip gnr_parts.hip gnr_retreat.hip gnr_support.hip gnr_balance.hip gnr_track.hip gnr_distance.hip gnr_tsdf.hip gnr_img.hip gnr_ingest.hip gnr_metrics.hip gnr_pack.cpp gnr_pack_dev.hip gnr_host_rng.cpp"
CFLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value -fno-slp-vectorize"
FLAGS="$CFLAGS -shared"

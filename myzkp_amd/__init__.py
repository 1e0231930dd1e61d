"""myzkp_amd -- MI355X-native MSM / NTT prover path for MyZKP (Python binding of the C ABI, include/mzk.h).

The product is the HIP library myzkp_amd/libmzk_hip.so; this module only marshals numpy limb arrays
into it (ctypes).  There is no CPU fallback: importing works without a GPU (so the ABI can be
inspected), but every compute call raises MzkError(MZK_E_NOGPU) unless a gfx950 device is present.
"""
from ._lib import (MzkError, lib, FIELD_FR, FIELD_M128, FIELD_FQ, FIELD_M64, FIELD_M64X3, LIMBS, MODULUS, init, shutdown, set_workspace_budget, trim_workspace, workspace_bytes, init_devices, ctx_count, ctx_select, shard_range, msm_g1_multi, SrsMulti, ntt_multi, ntt_multi_dev, LAYOUT_CONTIGUOUS, LAYOUT_CYCLIC,
                   ntt, intt, ntt_batch, coset_lde, coset_lde_batch, poly_scale, fft_multiply, fast_multiply, root_of_unity, msm_g1,
                   kzg_setup_g1, kzg_commit, kzg_open, kzg_batch_open, kzg_prove_degree_bound, fri_fold, Srs, MerkleTree, merkle_commit_field, merkle_commit_field_batch, merkle_open_multi, fri_commit, fri_prove, fri_proof_layout_gl, fri_prove_gl, fri_unpack_proof_gl, gemini_split_fold, gemini_split_fold_dev, sumcheck_sum, sumcheck_product_layout, sumcheck_frame_header, sumcheck_product_unpack, sumcheck_product_prove, mle_evals_from_coeffs, fri_proof_layout, fri_unpack_proof, fast_coset_divide, fast_coset_divide_batch_dev, fast_zerofier, fast_evaluate, fast_interpolate, fast_interpolate_batch, fast_interpolate_batch_dev, mpoly_term_table, mpoly_compose_plan, mpoly_compose, mpoly_compose_dev, poly_lincomb, poly_lincomb_dev, poly_div_roots, poly_div_roots_dev, stark_plan, StarkDims, stark_proof_layout, stark_unpack_proof, Stark, msm_g2, kzg_setup_g2, g2_points_to_array, array_to_g2_points, to_limbs, from_limbs, points_to_array,
                   rs_generator_poly, rs_encode, rs_encode_dev, rs_encode_view_dev, rs_syndromes, rs_syndromes_dev, rs_decode, rs_decode_dev, rs2d_encode, rs2d_encode_dev, rs2d_decode, rs2d_decode_dev, RS_NONE,
                   das_plan, das_commit, das_commit_dev, DasGrid, DAS_PATH_MAX, DAS_OUT_OF_RANGE,
                   rescue_plan, RescuePrime, RESCUE_MAX_M, RESCUE_MAX_ROUNDS,
                   array_to_points, exported_symbols, DECLARED_SYMBOLS)

__all__ = ["MzkError", "lib", "FIELD_FR", "FIELD_M128", "FIELD_FQ", "FIELD_M64", "FIELD_M64X3", "LIMBS", "MODULUS", "init", "shutdown", "init_devices", "ctx_count", "ctx_select", "shard_range", "msm_g1_multi", "SrsMulti", "ntt_multi", "ntt_multi_dev", "LAYOUT_CONTIGUOUS", "LAYOUT_CYCLIC",
           "ntt", "intt", "ntt_batch", "coset_lde", "coset_lde_batch", "poly_scale", "fft_multiply", "fast_multiply", "root_of_unity", "msm_g1",
           "kzg_setup_g1", "kzg_commit", "kzg_open", "kzg_batch_open", "kzg_prove_degree_bound", "fri_fold", "Srs", "MerkleTree", "merkle_commit_field", "merkle_commit_field_batch", "merkle_open_multi", "fri_commit", "fri_prove", "fri_proof_layout_gl", "fri_prove_gl", "fri_unpack_proof_gl", "gemini_split_fold", "gemini_split_fold_dev", "sumcheck_sum", "sumcheck_product_layout", "sumcheck_frame_header", "sumcheck_product_unpack", "sumcheck_product_prove", "mle_evals_from_coeffs", "fri_proof_layout", "fri_unpack_proof", "fast_coset_divide", "fast_coset_divide_batch_dev", "fast_zerofier", "fast_evaluate", "fast_interpolate", "fast_interpolate_batch", "fast_interpolate_batch_dev", "mpoly_term_table", "mpoly_compose_plan", "mpoly_compose", "mpoly_compose_dev", "poly_lincomb", "poly_lincomb_dev", "poly_div_roots", "poly_div_roots_dev", "stark_plan", "StarkDims", "stark_proof_layout", "stark_unpack_proof", "Stark", "msm_g2", "kzg_setup_g2", "g2_points_to_array", "array_to_g2_points", "to_limbs", "from_limbs", "points_to_array",
           "rs_generator_poly", "rs_encode", "rs_encode_dev", "rs_encode_view_dev", "rs_syndromes", "rs_syndromes_dev", "rs_decode", "rs_decode_dev", "rs2d_encode", "rs2d_encode_dev", "rs2d_decode", "rs2d_decode_dev", "RS_NONE",
           "das_plan", "das_commit", "das_commit_dev", "DasGrid", "DAS_PATH_MAX", "DAS_OUT_OF_RANGE",
           "rescue_plan", "RescuePrime", "RESCUE_MAX_M", "RESCUE_MAX_ROUNDS",
           "array_to_points", "exported_symbols", "DECLARED_SYMBOLS"]

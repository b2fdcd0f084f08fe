#!/usr/bin/env python3
"""tests/golden/refpins_golden.npz -- what the reference's own compiled code (oracle/_ref: the NNoM + CMSIS-NN build, the CMSIS-DSP
Q15 routines, firmware/src/audio/mfcc.c) answers on the inputs of the tests pinned to it, so that those tests hold where oracle/_ref
cannot be built (tests/refpins.py). The pinned tests themselves are run here with the live libraries, recording instead of
checking the recording, their own assertions included. Run where the reference's sources are at hand (oracle/Makefile REF), after
build():  python tests/golden/gen_fixtures_refpins.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
from oracle import oracle  # noqa: E402
import refpins  # noqa: E402


if __name__ == "__main__":
    oracle.build()
    assert oracle.have_ref() and oracle.have_q15_ref() and oracle.have_f32_ref(), "oracle/_ref is incomplete: the reference's sources are needed"
    from edison_amd import _lib
    import test_gpu_parity
    import test_oracle
    import test_oracle_refpins as R
    lib, model, q15, f32 = _lib.lib(), oracle.Model(), oracle.cmsis_q15_ref(), oracle.mfcc_f32_ref()
    refpins.RECORD = {}
    test_oracle.test_oracle_cnn_matches_reference_build(oracle, model)
    refpins.outputs("gpu_cnn_reference_build", lambda: oracle.nnom_ref_batch(test_gpu_parity.cnn_reference_build_inputs()))
    R.test_q15_oracle_stages_equal_the_reference_routines(oracle, q15)
    R.test_sqrt_q31_restatement_equals_the_reference_on_a_sweep(oracle, q15)
    R.test_variant_d_dct_matrix_equals_the_reference(lib, oracle, f32)
    R.test_variant_d_mel_filterbank_equals_the_reference(lib, oracle, f32)
    R.test_variant_d_transform_tables_come_from_the_reference_routine(oracle, f32)
    R.test_variant_d_restatement_equals_the_reference_mfcc_compute(oracle, f32)
    R.test_output_filter_class_choice_equals_arm_max_f32(oracle, f32)
    np.savez_compressed(refpins.PATH, **refpins.RECORD)
    print("wrote %s: %d arrays, %d bytes" % (refpins.PATH, len(refpins.RECORD), os.path.getsize(refpins.PATH)))

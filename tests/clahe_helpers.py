"""tests/clahe_helpers.py -- TEST INFRASTRUCTURE ONLY: the low-contrast synthetic stream the CLAHE GPU tests share (streams, runners
and comparisons are those of tests/fe_harness.py; the reference-equalised twin of a stream is stream.map(clahe_ref.clahe))."""
CONTRAST = 0.12            # see test_a_low_contrast_stream_gets_its_features_back
STREAM = dict(seed=13, n_frames=26, motion_scale=3.0, contrast=CONTRAST)

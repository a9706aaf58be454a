"""Training of the MLP template interpolator (the reference's rvspecfit.nn):
`python -m rvspecfit_amd.nn.train_interpolator` is rvs_train_nn_interpolator."""

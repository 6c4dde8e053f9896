"""The C ABI's error behaviour from C (tests/c/abi_errors.c): every entry point of
include/ldm_sdf.h called with invalid arguments returns an error code and leaves a message in
ldm_last_error(); the host-only entry points (ABI version, workspace sizes, AdamW scalars, the
marching-cubes table, the one-launch training step's job table built from descriptors) work
without a GPU.  Here the checker is built with gcc against the product library; the same source
runs under host AddressSanitizer with `make -C latent-diffusion-models-for-shape-sdfs_amd/csrc
check-asan` (libldm_sdf_asan.so; log under profiles/)."""

from tests.c_checker import run_c_checker


def test_abi_errors_from_c(tmp_path):
    run_c_checker("abi_errors", tmp_path)

"""TEST INFRASTRUCTURE ONLY: install() puts the device-code simulator's engine (devsim.SimEngine: the product's LgarEngine with
tests/devsim in the HIP library's place) behind lgar_py_amd.model and lgar_py_amd.autograd, so that CPU tests run the model
surface, the autograd tape and the sharded training loop under gloo without a GPU.  Never imported by the product."""
from devsim import install  # noqa: F401

"""lgar_py_amd: MI355X-native many-column LGAR infiltration engine (hot path of LGAR-py / dpLGAR).

(`lgar-py_amd` at the repo root is a symlink to this directory: a hyphen cannot be imported.)
"""
from ._capi import ACC_NAMES, FMAX, LMAX, LgarError  # noqa: F401
from .baseflow import CatchmentBaseflow, catchment_baseflow  # noqa: F401
from .catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum  # noqa: F401
from .engine import EngineState, LgarEngine, LgarStatusError, TangentState, leaf_batch, leaf_tangent_batch  # noqa: F401
from .forcing import ForcingDirections, ForcingMap, scaled_forcing  # noqa: F401
from .network import (CatchmentNetwork, NetworkPools, manning_reach_parameters, muskingum_coefficients, network_route, network_route_mc,  # noqa: F401
                      network_route_pool, weir_pool_parameters)
from .scores import CatchmentScore, catchment_moments  # noqa: F401
from .snow import CatchmentSnow, catchment_snow, catchment_snow_directions  # noqa: F401
from .canopy import CatchmentCanopy, catchment_canopy, catchment_canopy_directions  # noqa: F401

__all__ = ["LgarEngine", "EngineState", "TangentState", "LgarError", "LgarStatusError", "leaf_batch", "leaf_tangent_batch", "CatchmentMap", "catchment_sum", "CatchmentRouting", "catchment_route", "CatchmentScore", "catchment_moments", "CatchmentNetwork", "network_route", "network_route_mc", "manning_reach_parameters", "NetworkPools", "network_route_pool", "weir_pool_parameters",
           "muskingum_coefficients", "CatchmentBaseflow", "catchment_baseflow", "CatchmentSnow", "catchment_snow", "catchment_snow_directions", "CatchmentCanopy", "catchment_canopy", "catchment_canopy_directions", "ForcingMap", "ForcingDirections", "scaled_forcing", "ACC_NAMES", "FMAX",
           "LMAX"]

"""ultraspy's Doppler module (DESIGN D24): colour and power Doppler on an ensemble of beamformed I/Q frames.  `ultraspy` is absent: the
names get_color_doppler_map and get_power_doppler_map are its own from memory, the arithmetic is this build's definition
(include/pbrt_hip.h) and parity with it is unpinned.  Its apply_wall_filter is not a step of its own here: the wall filter is an
argument of the autocorrelation (doppler_autocorr(frames, wall_filter=..., degree=...)), which never writes the filtered ensemble."""
from ..beamform import (doppler_autocorr, doppler_maps, get_color_doppler_map, get_power_doppler_map, nyquist_velocity,  # noqa: F401
                        wall_basis)

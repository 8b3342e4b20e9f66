"""ultraspy.beamformers.slsc (DESIGN D26): short-lag spatial coherence.  NOT one of ultraspy's beamformers -- the module sits beside
them so that a script finds every beamformer of this build in one place; the class and its arithmetic are this build's own."""
from ...beamform import ShortLagSpatialCoherence  # noqa: F401

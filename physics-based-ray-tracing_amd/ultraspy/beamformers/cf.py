"""ultraspy.beamformers.cf (DESIGN D26): delay-and-sum weighted by the coherence factor.  NOT one of ultraspy's beamformers -- the module
sits beside them so that a script finds every beamformer of this build in one place; the class and its arithmetic are this build's own."""
from ...beamform import CoherenceFactor  # noqa: F401

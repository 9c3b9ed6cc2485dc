"""fib_tf_amd — MI355X-native explicit time-stepper for 2D cardiac reaction-diffusion with the
config-dict / IonicModel / define() / run() API of siravan/fib_tf.  Python host code over a ctypes
C ABI (include/fibhip.h) into hand-written HIP kernels for gfx950; no TensorFlow, no CPU fallback.

    from fib_tf_amd.fenton import Fenton4v
    from fib_tf_amd.br import BeelerReuter
    from fib_tf_amd.court import Courtemanche
"""
from . import _lib                              # noqa: F401
from .ionic import IonicModel                   # noqa: F401
from .fenton import Fenton4v                    # noqa: F401
from .br import BeelerReuter                    # noqa: F401
from .court import Courtemanche                 # noqa: F401
from . import tips                              # noqa: F401  (TipRecorder, link: spiral tips recorded on the device)
from . import frames                            # noqa: F401  (FrameRecorder: the movie cube recorded on the device)
from . import stats                             # noqa: F401  (StatsRecorder: tissue statistics recorded on the device)
from . import spectrum                          # noqa: F401  (SpectrumRecorder: per-cell power spectra and dominant-frequency maps)
from . import beats                             # noqa: F401  (BeatRecorder: per-cell beat history, restitution and alternans maps)
from . import velocity                          # noqa: F401  (conduction-velocity maps and CV restitution, fitted on the device)
from . import leads                             # noqa: F401  (LeadRecorder: unipolar electrograms from the membrane current)
from . import potential                         # noqa: F401  (PotentialMapRecorder: unipolar electrograms at every site of a lattice)
from . import waves                             # noqa: F401  (WaveRecorder: excited domains labelled and counted on the device)
from . import stimulus                        # noqa: F401  (Stimulus, StimulusProgram: pacing protocols run on the device)
from . import triggers                          # noqa: F401  (Sensor, Trigger, TriggerProgram: triggered stimulation on the device)

__all__ = ['IonicModel', 'Fenton4v', 'BeelerReuter', 'Courtemanche']

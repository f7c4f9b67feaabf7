"""vqvae_amd -- MI355X-native training hot path of dhgrs/chainer-VQ-VAE behind a
Chainer-shaped Chain / FunctionNode surface.  Host = Python; all arithmetic =
hand-written HIP (gfx950) in libvqvae_hip.so reached through a C ABI."""
from . import _lib, backend, core, functions, links, optimizers, reporting  # noqa: F401
from .core import (Chain, ChainList, FunctionNode, Link, Parameter, Variable,  # noqa: F401
                   config, report, using_config)
from .codebook import CodebookMonitor  # noqa: F401
from .codebook_ema import EMACodebook  # noqa: F401
from .codebook_init import KMeansCodebookInit, kmeans_init  # noqa: F401
from .optimizers import GradientClipping, GradientNorms, NonFiniteGuard  # noqa: F401
from .net import VAE, ConditionEmbed, Encoder  # noqa: F401
from .updaters import (VQVAE_ParallelUpdater, VQVAE_StandardUpdater,  # noqa: F401
                       concat_examples)
from .utils import VQ, ExponentialMovingAverage, MuLaw, StraightThrough, straight_through  # noqa: F401
from .wavenet import ResidualBlock, ResidualNet, WaveNet  # noqa: F401
from .generation import DeviceUniforms, LatentCondition  # noqa: F401
from .corpus import CorpusView, ResidentCorpus, ResidentCorpusIterator  # noqa: F401
from .ingest import (DeviceIngest, corpus_files, read_wav, resample_taps, write_wav)  # noqa: F401
from .frontend import (LatentCodes, condition_many, encode_many, frontend_many, plan_chunks)  # noqa: F401
from .metrics import MelConfig, RaggedFeatures, compare_many, features_many  # noqa: F401
from .pitch import PitchConfig, RaggedPitch, compare_pitch_many, pitch_many  # noqa: F401
from .scoring import Scores, evaluate_many, score_many  # noqa: F401
from .scoring_mol import MolScores, evaluate_many_mol, score_many_mol  # noqa: F401
from .alignment import Alignment, align_many, compare_aligned_many  # noqa: F401
from .codestats import (CodeComparison, CodeRuns, CodeStats, code_stats, collapse_many,  # noqa: F401
                        compare_codes_many)
from .speakerid import (RaggedSpeakerFeatures, SpeakerModels, SpeakerScores, fit_speakers,  # noqa: F401
                        identify_many, score_speakers, speaker_features)
from .segmental import SegmentalCodes, segment_latents, segment_many  # noqa: F401
from .abx import (ABXPlan, ABXScores, Frames, Items, PairDistances, abx_many, code_table, pair_distances,  # noqa: F401
                  plan_abx)
from .synthesis import synthesize, synthesize_many  # noqa: F401
from .reporting import LogReport, PlotReport, PrintReport  # noqa: F401

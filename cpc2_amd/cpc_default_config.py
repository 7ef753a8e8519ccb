"""The architecture / optimisation / augmentation flags shared by every command line of the package.

Same flags, types, choices and defaults as the reference's cpc/cpc_default_config.py:13-162 -- all of them, the
augmentation group included: cpc2_amd.train builds additive / natural_reverb / time_dropout (data_augmentation.py) and
pitch_wsola (a choice of --augment_type the reference does not have: a pitch shift by this package's own definition) and
freeverb (likewise: the Freeverb network behind sox's reverb, by this package's own definition, with ReverbAugment's draw) and
bandreject_sinc (likewise: a Kaiser-windowed sinc band-reject filter, by this package's own definition, with BandrejectAugment's draw), and
refuses the sox-based types with a message (train.py, refuseUnsupported), and checkpoint_args.json carries the same keys as a reference run, so that either side can resume the other's run."""
import argparse

NAMING_CONVENTIONS = ['full_seedlings', 'no_speaker', 'id_spkr_onset_offset', 'spkr-id', 'spkr-id-nb',
                      'id_spkr_onset_offset_spkr_onset_offset', 'spkr_id_nb']
AUGMENT_TYPES = ['none', 'bandreject', 'pitch', 'pitch_deropout', 'pitch_quick', 'additive', 'artificial_reverb',
                 'time_dropout', 'artificial_reverb_dropout', 'natural_reverb', 'pitch_wsola', 'freeverb', 'bandreject_sinc']


def get_default_cpc_config():
    """The namespace of defaults (cpc_default_config.py:8-10)."""
    return set_default_cpc_config(argparse.ArgumentParser()).parse_args([])


def set_default_cpc_config(parser):
    g = parser.add_argument_group('Architecture configuration', description="What the model, the criterion and the "
                                  "optimiser are built from.")
    g.add_argument('--hiddenEncoder', type=int, default=256, help='Width of the encoder.')
    g.add_argument('--hiddenGar', type=int, default=256, help='Width of the context (auto-regressive) network.')
    g.add_argument('--nPredicts', type=int, default=12, help='Prediction steps of the CPC loss.')
    g.add_argument('--negativeSamplingExt', type=int, default=128, help='Negative samples per positive.')
    g.add_argument('--optimizer', type=str, default='adam', choices=['adam', 'sgd'],
                   help='adam (fused flat Adam) or sgd (fused flat SGD, momentum 0.9).')
    g.add_argument('--learningRate', type=float, default=2e-4)
    g.add_argument('--schedulerStep', type=int, default=-1,
                   help='Halve the learning rate every this many epochs (default: never).')
    g.add_argument('--schedulerRamp', type=int, default=None,
                   help='Linear warm-up of the learning rate over this many epochs.')
    g.add_argument('--beta1', type=float, default=0.9, help='Adam beta1.')
    g.add_argument('--beta2', type=float, default=0.999, help='Adam beta2.')
    g.add_argument('--epsilon', type=float, default=1e-08, help='Adam epsilon.')
    g.add_argument('--sizeWindow', type=int, default=20480, help='Samples per window.')
    g.add_argument('--nEpoch', type=int, default=200, help='Epochs to run.')
    g.add_argument('--samplingType', type=str, default='samespeaker',
                   choices=['samespeaker', 'uniform', 'samesequence', 'sequential', 'temporalsamespeaker'],
                   help='Which windows share a batch (the negatives come from the batch).')
    g.add_argument('--nLevelsPhone', type=int, default=1, help='(supervised mode) layers of the phone classifier.')
    g.add_argument('--cpc_mode', type=str, default=None, choices=['reverse', 'bert', 'none'], help='CPC variants.')
    g.add_argument('--encoder_type', type=str, choices=['cpc', 'mfcc', 'lfb'], default='cpc',
                   help='Only cpc (the raw-waveform encoder) is built here.')
    g.add_argument('--normMode', type=str, default='layerNorm', choices=['instanceNorm', 'ID', 'layerNorm', 'batchNorm'],
                   help='Normalisation of the encoder (only layerNorm is built here).')
    g.add_argument('--onEncoder', action='store_true', help='(supervised mode) classify the encoder output.')
    g.add_argument('--random_seed', type=int, default=None, help='Seed of every generator (drawn when absent).')
    g.add_argument('--arMode', default='LSTM', choices=['GRU', 'LSTM', 'RNN', 'no_ar', 'transformer'],
                   help='Context network.')
    g.add_argument('--nLevelsGRU', type=int, default=1, help='Layers of the context network.')
    g.add_argument('--rnnMode', type=str, default='transformer',
                   choices=['transformer', 'RNN', 'LSTM', 'linear', 'ffd', 'conv4', 'conv8', 'conv12',
                            'transformer_adaptive_span'], help='Prediction network.')
    g.add_argument('--dropout', action='store_true', help='Dropout after the prediction network.')
    g.add_argument('--abspos', action='store_true', help='Absolute positions in a transformer.')
    g.add_argument('--multihead_rnn', action='store_true',
                   help='One prediction network with nPredicts heads instead of nPredicts networks.')
    g.add_argument('--adapt_span_loss', type=float, default=2e-6)
    g.add_argument('--transformer_pruning', type=int, default=0)
    g.add_argument('--naming_convention', type=str, default=None, choices=[None] + NAMING_CONVENTIONS,
                   help='How file names encode (speaker, order); needed by temporalsamespeaker sampling.')
    g.add_argument('--no_artefacts', action='store_true',
                   help='Move a window that would run over the end of its recording to the start of the next one.')
    g.add_argument('--mask_prob', type=float, default=0.0, help='Probability of a span mask on the encoded features.')
    g.add_argument('--mask_length', type=int, default=10, help='Frames per span mask.')
    g.add_argument('--signal_quality_path', type=str, default=None,
                   help='Directory of per-file signal quality estimates (.pt) for the quality-weighted loss.')
    g.add_argument('--signal_quality_step', type=int, default=1600, help='Samples per signal quality estimate.')
    g.add_argument('--signal_quality_mode', type=str, choices=['snr', 'c50', 'snr_c50'], default='snr')
    g.add_argument('--growth_rate', type=float, default=10, help='Steepness of the quality weighting sigmoid.')
    g.add_argument('--inflection_point_x', type=float, default=0.5, help='Centre of the quality weighting sigmoid.')
    g.add_argument('--n_skipped', type=int, default=0, help='Time steps skipped before the first prediction.')
    g.add_argument('--no_speaker', action='store_true', help='Collapse every speaker into one.')
    a = parser.add_argument_group('Data augmentation configuration',
                                  description="Device-side augmentation of the past / future half (cpc2_amd/data_augmentation.py): "
                                  "additive, natural_reverb, time_dropout, pitch_wsola and none are built, alone or combined; the "
                                  "sox-based types are parsed for checkpoint compatibility and refused by name.  pitch_wsola "
                                  "shifts the pitch by up to --shift_max cents (a WSOLA stretch and a sinc resampling: this "
                                  "package's definition, not sox's).  freeverb reverberates without "
                                  "impulse responses (the Freeverb comb / all-pass network with the room size drawn per window: "
                                  "this package's definition, agreement with sox's reverb unmeasured).  bandreject_sinc rejects one "
                                  "frequency band per window, drawn on the mel scale and scaled by --bandreject_scaler (a "
                                  "Kaiser-windowed sinc FIR in float64: this package's definition, agreement with sox's sinc "
                                  "unmeasured, no dither).")
    a.add_argument('--noise_extension', type=str, default='.wav')
    a.add_argument('--augment_future', action='store_true')
    a.add_argument('--augment_past', action='store_true')
    a.add_argument('--augment_type', type=str, choices=AUGMENT_TYPES, nargs='+')
    a.add_argument('--bandreject_scaler', type=float, default=1.0,
                   help='bandreject_sinc: the band is at most 27 x this many of 256 mel steps wide; from 0 to 256 / 27.')
    a.add_argument('--t_ms', type=int, default=100)
    a.add_argument('--pathDBNoise', type=str, default=None)
    a.add_argument('--pathSeqNoise', type=str, default=None)
    a.add_argument('--past_equal_future', action='store_true')
    a.add_argument('--pathImpulseResponses', type=str, default=None)
    a.add_argument('--impulse_response_prob', type=float, default=1.0)
    a.add_argument('--shift_max', type=float, default=300,
                   help='pitch_wsola: cents drawn from [-shift_max, shift_max), a whole number from 1 to 1200.')
    a.add_argument('--min_snr_in_db', type=float, default=5.0)
    a.add_argument('--max_snr_in_db', type=float, default=20.0)
    a.add_argument('--ir_sample_rate', type=int, default=16000)
    a.add_argument('--temporal_additive_noise', action='store_true')
    a.add_argument('--meta_aug', action='store_true')
    a.add_argument('--meta_aug_type', type=str, choices=['none', 'natural_reverb', 'freeverb'], nargs='+')
    a.add_argument('--ir_batch_wise', action='store_true')
    a.add_argument('--meta_ir_batch_wise', action='store_true')
    return parser

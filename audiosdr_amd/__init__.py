"""audiosdr_amd -- batched AudioSDR update() demodulation chain on AMD Instinct MI355X.

The product is libasdr_hip.so (hand-written HIP kernels for gfx950 behind the C ABI of
include/asdr.h).  This package is only a thin ctypes mirror of that ABI whose class,
`AudioSDRBatch`, keeps the reference's method names (AudioSDR.h:88-156) so that test code
reads like reference usage.  There is no CPU fallback: if the library or a HIP device is
missing, construction raises.
"""
from .binding import (STREAM_BATCH, AGCfast, AGCmedium, AGCoff, AGCslow, ALL, AMmode, BLOCK, CW_LSBmode, CW_USBmode, LSBmode, SAMmode,
                      TAPS, USBmode, WSPRmode, AudioSDRBatch, AsdrError, audio2100, audio2300, audio2500, audio2700,
                      audio2900, audio3100, audio3300, audioAM, audioBypass, audioCW, audioWSPR, library_path,
                      library_sha256, load_library, host_alloc, host_free, state_field, state_record_bytes, state_record_fields)
from .front import (NO_DEVICE, AudioGrabberComplex256Batch, AudioIQgeneratorBatch, AudioSDRpreProcessorBatch,  # noqa: E402
                    FRONT_EXPORTS)
from .tuner import (IQ_CORRECTION_DTYPE, IQ_IDENTITY, IQ_STATS_DTYPE, TUNER_EXPORTS, TUNER_STATE_DTYPE, TunerBank,  # noqa: E402
                    design_channel_filter, estimate_iq_correction, fastconv_ratio, rate_ratio, spectrum_frequencies,
                    suggest_decimation, suggest_fft_decimation, tuner_channel_field, tuner_channel_record_fields)
from .gate import GATE_EXPORTS, GATE_STATE_DTYPE, GATE_TILE, AudioGate, energy_from_dbfs  # noqa: E402
from .resample import (RESAMPLE_DEFAULT_RATES, RESAMPLE_EXPORTS, RESAMPLE_FS_IN, RESAMPLE_STATE_SAMPLES,  # noqa: E402
                       AudioResampler)
from .codec import (CODEC_EXPORTS, CODEC_KINDS, CODEC_MAX_SAMPLES, CODEC_STATE_DTYPE, AudioCodec, codec_decode,  # noqa: E402
                    codec_row_bytes)
from .spectrogram import (SPECTROGRAM_EXPORTS, SPECTROGRAM_KINDS, SPECTROGRAM_MAX_SAMPLES, SPECTROGRAM_SIZES,  # noqa: E402
                          SPECTROGRAM_WINDOWS, AudioSpectrogram)
from .fm import (FM_CHUNK_BLOCKS, FM_EXPORTS, FM_MAX_NOISE, FM_NARROW_ROWS, FM_ROWS, FM_STATE_DTYPE,  # noqa: E402
                 FM_WIDE_CHANNELS, FmDemodulator, fm_deemphasis_from_tau_us, fm_gain_from_deviation)
from .tone import (CTCSS_TONES, TONE_ANY, TONE_EXPORTS, TONE_MAX_TONES, TONE_PASS, TONE_ROWS, TONE_STATE_DTYPE,  # noqa: E402
                   TONE_WAVE_ROWS, ToneSquelch, tone_highpass_design, tone_min_power)
from .dcs import (DCS_ANY, DCS_CODES, DCS_EXPORTS, DCS_MAX_CODES, DCS_NARROW_ROWS, DCS_PASS, DCS_ROWS, DCS_STATE_DTYPE,  # noqa: E402
                  DCS_WIDE_CHANNELS, DcsSquelch, dcs_word)
from .packet import (PACKET_EXPORTS, PACKET_FRAME_DTYPE, PACKET_MAX_PAYLOAD, PACKET_MAX_RING, PACKET_NARROW_ROWS,  # noqa: E402
                     PACKET_ROWS, PACKET_STATE_DTYPE, PACKET_WIDE_CHANNELS, PacketDecoder, packet_fcs, packet_format_address)
from .cw import (CW_EVENT_DTYPE, CW_EXPORTS, CW_FLAG_UNKNOWN, CW_MAX_RING, CW_NARROW_ROWS, CW_ROWS, CW_STATE_DTYPE,  # noqa: E402
                 CW_WIDE_CHANNELS, CwDecoder, cw_pitch_step)

__all__ = [n for n in dir() if not n.startswith("_")]

"""params_uniform (include/asdr.h asdr_params_uniform_groups, asdr_host.cpp): a settings group of consecutive channels whose
parameter rows are equal has its large launches carry the row as launch constants.  The host keeps that knowledge incrementally:
one row comparison per row a per-channel setter changed, a pass over a group's rows after a broadcast setter or a schedule rebuild,
nothing at a flush with no setter in front of it.  Runs WITHOUT a GPU through a control-plane-only batch (ASDR_NO_DEVICE)."""


def _state(b):
    b.control_plane_flush()
    return b.params_uniform_groups()


def test_flag_follows_broadcast_and_per_channel_setters(A):
    n = 1024
    b = A.AudioSDRBatch(n, device=-1)
    assert _state(b)[0] == 1                               # power-on settings: one group, one row
    b.setDemodMode(A.USBmode); b.enableAudioFilter()       # C2's settings, by broadcast
    assert _state(b)[0] == 1
    b.setOutputGain(0.7, ch=37)                            # one row differs
    assert _state(b)[0] == 0
    b.setInputGain(0.5)                                    # a broadcast of ANOTHER field: channel 37 still differs
    assert _state(b)[0] == 0
    b.setOutputGain(0.5)                                   # a broadcast of that field: equal again
    assert _state(b)[0] == 1
    b.setNoiseBlankerThresholdDb(10.0, ch=5); b.setOutputGain(0.7, ch=9)
    assert _state(b)[0] == 0
    b.setOutputGain(0.5, ch=9)                             # one of the two put back: channel 5 still differs
    assert _state(b)[0] == 0
    b.setNoiseBlankerThresholdDb(10.0)
    assert _state(b)[0] == 1
    b.setOutputGain(0.25, ch=0)                            # the group's first row (what the others are compared with)
    assert _state(b)[0] == 0
    b.setOutputGain(0.5, ch=0)
    assert _state(b)[0] == 1
    b.setOutputGain(0.25, ch=0); b.setOutputGain(0.25)     # first row, then everybody: equal
    assert _state(b)[0] == 1
    b.close()


def test_flag_is_recomputed_only_after_a_setter(A):
    n = 4096
    b = A.AudioSDRBatch(n, device=-1)
    g, rows = _state(b)
    assert g == 1 and rows == n                            # the first flush passes over the group once
    for _ in range(3):                                     # no setter in between: nothing is compared
        assert _state(b) == (1, rows)
    b.setOutputGain(0.7, ch=37)                            # a per-channel setter: ONE comparison
    assert _state(b) == (0, rows + 1)
    assert _state(b) == (0, rows + 1)
    b.setOutputGain(0.5, ch=37); b.setOutputGain(0.6, ch=38); b.setOutputGain(0.5, ch=38)   # two rows refilled: two comparisons
    assert _state(b) == (1, rows + 3)
    b.setOutputGain(0.5)                                   # a broadcast setter refills every row: one pass
    assert _state(b) == (1, rows + 3 + n)
    assert _state(b) == (1, rows + 3 + n)
    b.setDemodMode(A.USBmode, ch=100)                      # the schedule is rebuilt; the LSB group's channels are no longer consecutive, so
    g, rows2 = _state(b)                                   # its launches are not direct ones: no group carries the flag, nothing to compare
    assert g == 0 and rows2 == rows + 3 + n
    assert _state(b) == (0, rows2)
    b.close()


def test_two_groups_carry_their_own_flags(A):
    """512 LSB and 1,024 SAM channels: two kernel kinds, each ONE settings group of consecutive channels and each uniform in itself."""
    n = 1536
    b = A.AudioSDRBatch(n, device=-1)
    for c in range(512, n):
        b.setDemodMode(A.SAMmode, ch=c)
    st = b.control_plane_flush()
    assert st["waves_plain"] == 64 and st["waves_sam"] == 128
    assert b.params_uniform_groups()[0] == 2
    b.setOutputGain(0.7, ch=1000)                          # a SAM channel: its group only
    assert _state(b)[0] == 1
    b.setOutputGain(0.7, ch=3)                             # ... and the other group
    assert _state(b)[0] == 0
    for c in range(512, n):
        b.setOutputGain(0.7, ch=c)                         # the SAM group is equal again, with a row unlike the other group's
    assert _state(b)[0] == 1
    b.setOutputGain(0.7, ch=3); b.setOutputGain(0.5, ch=3)
    assert _state(b)[0] == 2
    b.close()

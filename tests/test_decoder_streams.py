"""Host: the decoder's stream / event helper (``decoder._Streams``) with recording fake events and
fake streams — which event is recorded and waited on which stream by each ordering, the same
sequence from the device-scope flavour (raw handles) and the default one (stream objects), and
nothing at all on a single stream."""
import pytest

from scflow_amd.decoder import _Streams

HANDLES = {"main": 0x1000, "side": 0x2000}


class FakeStream:
    def __init__(self, name):
        self.name, self.cuda_stream = name, HANDLES[name]


class FakeEvent:
    """record(s) / wait(s) as ops.SyncEvent (s: a raw handle) and torch.cuda.Event (s: a stream)
    have them; logs (event, call, stream name, whether s was a raw handle)."""

    def __init__(self, name, log):
        self.name, self.log = name, log

    def _note(self, call, s):
        raw = isinstance(s, int)
        name = {v: k for k, v in HANDLES.items()}[s] if raw else s.name
        self.log.append((self.name, call, name, raw))

    def record(self, s):
        self._note("record", s)

    def wait(self, s):
        self._note("wait", s)


def make(raw, two=True, events=True):
    log = []
    main = FakeStream("main")
    side = FakeStream("side") if two else main
    evs = tuple(FakeEvent(n, log) for n in ("fork", "join", "mark")) if events else None
    return _Streams(main, side, evs, raw=raw), log


def run_all(st):
    st.fork()
    st.join()
    st.mark_side()
    st.wait_side_mark()
    st.wait_side_mark()  # the mark is waited on once per iteration; recorded once here


WANT = [("fork", "record", "main"), ("fork", "wait", "side"),      # side waits for main
        ("join", "record", "side"), ("join", "wait", "main"),      # main waits for side
        ("mark", "record", "side"),                                # mark_side
        ("mark", "wait", "main"), ("mark", "wait", "main")]        # wait_side_mark


@pytest.mark.parametrize("raw", [True, False])
def test_streams_orderings(raw):
    st, log = make(raw)
    assert st.two and st.side is not st.main
    assert (st.h_main, st.h_side) == (HANDLES["main"], HANDLES["side"])
    run_all(st)
    assert [e[:3] for e in log] == WANT
    # the device-scope flavour is given raw handles, the default one the stream objects
    assert all(e[3] == raw for e in log)


def test_streams_flavours_issue_the_same_sequence():
    (a, la), (b, lb) = make(True), make(False)
    run_all(a)
    run_all(b)
    assert [e[:3] for e in la] == [e[:3] for e in lb] == WANT


@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("two,events", [(False, True), (False, False), (True, False)])
def test_streams_single_stream_issues_nothing(raw, two, events):
    st, log = make(raw, two=two, events=events)
    assert not st.two and st.side is st.main and st.h_side == st.h_main
    run_all(st)
    assert log == []

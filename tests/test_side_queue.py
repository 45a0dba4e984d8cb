"""The fork protocol of the two-stream schedule (network._SideQueue) against a stub net that logs every event it
makes, records and waits for.  No GPU and no library: the streams carry only a handle, and _lib.pin_stream is Python."""
import pytest

from lisec_amd import _lib
from lisec_amd.network import _SideQueue

MAIN, SIDE = 11, 22


class Stream:
    def __init__(self, handle):
        self.cuda_stream = handle


class StubNet:
    def __init__(self):
        self.log, self.made = [], []

    def _new_event(self):
        self.made.append(object())
        return self.made[-1]

    def _record(self, ev, stream):
        self.log.append(("record", ev, stream.cuda_stream))

    def _wait(self, ev, stream):
        self.log.append(("wait", ev, stream.cuda_stream))


@pytest.fixture
def queue():
    prev = _lib.pin_stream(MAIN)
    net = StubNet()
    q = _SideQueue(net, Stream(MAIN), Stream(SIDE))
    q.begin()
    yield net, q
    _lib.pin_stream(prev)


def closure(net, name):
    return lambda: net.log.append(("ran", name, _lib.current_stream()))


def test_marked_fork_is_waited_for_and_closures_run_in_order_on_the_side_handle(queue):
    net, q = queue
    q.mark_fork()
    marked = net.made[0]
    q.defer(closure(net, "a"))
    q.defer(closure(net, "b"))
    assert net.log == [("record", marked, MAIN)]            # nothing crosses before the flush
    q.flush()
    assert net.log == [("record", marked, MAIN), ("wait", marked, SIDE), ("ran", "a", SIDE), ("ran", "b", SIDE)]
    assert len(net.made) == 1                               # the flush recorded no event of its own
    assert _lib.current_stream() == MAIN and q.pending == [] and q.marked == []


def test_unmarked_flush_records_one_event_on_main_then_waits_on_side(queue):
    net, q = queue
    q.run(closure(net, "a"))
    ev = net.made[0]
    assert net.log == [("record", ev, MAIN), ("wait", ev, SIDE), ("ran", "a", SIDE)]
    assert len(net.made) == 1


def test_empty_flush_logs_nothing_and_keeps_the_mark(queue):
    net, q = queue
    q.flush()
    assert net.log == [] and net.made == []
    q.mark_fork()
    marked = net.made[0]
    q.flush()                                               # nothing pending: the mark is not consumed
    assert net.log == [("record", marked, MAIN)] and q.marked == [marked]
    q.run(closure(net, "a"))
    assert net.log[1:] == [("wait", marked, SIDE), ("ran", "a", SIDE)] and len(net.made) == 1


def test_a_given_event_is_marked_instead_of_one_of_the_pool(queue):
    net, q = queue
    named = object()
    q.mark_fork(named)
    q.run(closure(net, "a"))
    assert net.log == [("record", named, MAIN), ("wait", named, SIDE), ("ran", "a", SIDE)]
    assert net.made == [] and q.events == []


def test_a_raising_closure_leaves_the_pin_restored_and_nothing_pending(queue):
    net, q = queue

    def boom():
        raise ValueError("boom")

    q.defer(closure(net, "a"))
    q.defer(boom)
    q.defer(closure(net, "never"))
    with pytest.raises(ValueError):
        q.flush()
    assert _lib.current_stream() == MAIN and q.pending == []
    assert [e[:2] for e in net.log if e[0] == "ran"] == [("ran", "a")]


def test_join_records_on_side_and_waits_on_main(queue):
    net, q = queue
    ev = object()
    q.join(ev)
    assert net.log == [("record", ev, SIDE), ("wait", ev, MAIN)]


def one_pass(net, q):
    q.begin()
    q.run(closure(net, "a"))
    q.mark_fork()
    q.defer(closure(net, "b"))
    q.run(closure(net, "c"))
    q.run(closure(net, "d"))


def test_begin_reuses_the_events_of_the_pass_before(queue):
    net, q = queue
    one_pass(net, q)
    first, pool = list(net.log), list(q.events)
    assert len(pool) == 3 == len(net.made)
    del net.log[:]
    one_pass(net, q)
    assert net.log == first                                 # the same event objects, in the same roles
    assert len(q.events) == 3 == len(net.made) and all(x is y for x, y in zip(q.events, pool))


def test_begin_can_name_another_main_stream(queue):
    net, q = queue
    q.begin(Stream(33))
    q.run(closure(net, "a"))
    assert net.log[0] == ("record", net.made[0], 33)

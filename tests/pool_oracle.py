"""Plain-Python statement of the online-hard-mining pool's rules (csrc/pool.hip ``pool_select_kernel`` and
``online.OnlineHardPool.replay``).  No torch, no native library; tests/test_pool_oracle_host.py pins it against what the
reference's ``save_data_online`` / ``OnlineHMData`` did on recorded key streams (tests/golden/online_pool_known.npz) and
against the project's own rules where the reference is not well defined; tests/test_online_pool_gpu.py compares the kernels
with it.

Select, per call, samples in order i = 0 .. B-1:
  * a key that is NaN or infinite: slot -1, nothing changes;
  * pool not full: the next free slot (= count);
  * pool full (capacity > 0): the entry with the least (key, seq) -- of equal keys the oldest -- gives up its slot, unless the
    new key is STRICTLY smaller than that entry's key (a key equal to the minimum is accepted, as bisect.bisect places it
    behind its equals); capacity 0: slot -1;
  * a stored sample gets seq = next, and next grows by one (skipped samples use no sequence number);
  * when a later sample of the call takes the slot an earlier sample of the call was given, the earlier one's slot becomes -1.
Replay: slots ascending by (key, seq); ``order[-int(rate * n):]`` taken literally (a product of 0 selects everything)."""
import math


class PoolOracle:
    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.keys = [None] * self.capacity            # per slot; None: never written
        self.seq = [None] * self.capacity
        self.payload = [None] * self.capacity         # whatever the caller attaches to a stored sample (an id, tensors)
        self.count = 0
        self.next = 0

    def clear(self):
        self.count = 0
        self.next = 0

    def add(self, keys, payloads=None):
        """Returns the slots of the call (after the in-call rule)."""
        slots = []
        for i, key in enumerate(keys):
            key = float(key)
            slot = -1
            if math.isfinite(key):
                if self.count < self.capacity:
                    slot = self.count
                    self.count += 1
                elif self.capacity > 0:
                    m = min(range(self.capacity), key=lambda j: (self.keys[j], self.seq[j]))
                    if not key < self.keys[m]:
                        slot = m
            if slot >= 0:
                self.keys[slot], self.seq[slot] = key, self.next
                self.payload[slot] = None if payloads is None else payloads[i]
                self.next += 1
                slots = [-1 if s == slot else s for s in slots]
            slots.append(slot)
        return slots

    def stored(self):
        """Payloads of the occupied slots, by slot."""
        return [self.payload[j] for j in range(self.count)]

    def replay_slots(self, rate=1.0):
        order = sorted(range(self.count), key=lambda j: (self.keys[j], self.seq[j]))
        return order[-int(rate * len(order)):]

    def replay_batches(self, perm, batch_size=1, rate=1.0):
        """Slot lists of the batches for a given permutation of range(len(replay_slots(rate))); the incomplete last one dropped."""
        chosen = self.replay_slots(rate)
        assert sorted(perm) == list(range(len(chosen)))
        return [[chosen[p] for p in perm[j * batch_size:(j + 1) * batch_size]] for j in range(len(chosen) // batch_size)]

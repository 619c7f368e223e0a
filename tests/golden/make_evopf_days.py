"""Writes tests/golden/evopf_days.npz: 8 days of the system load and price files the reference ships next to its loaders.

    python tests/golden/make_evopf_days.py DIR        # DIR holds demand.pickle and price.pickle (rpo/env/electrical_grid/data/crawlers)

demand.pickle: a dict whose "value" is the hourly system load (731 days); price.pickle: a dict whose "SYS" is the hourly system
price (668 days; it has negative hours).  Day d of the fixture is hours [24 d, 24 d + 24) of the load and hours [24 d, 24 d + 48)
of the price -- the day and the look-ahead past midnight, what the reference's real-day mode reads (price.py:35).  The days: the
one that holds the lowest price of the file (a negative one), and seven spread evenly over the span both files cover.
Arrays: load float64 [8, 24], price float64 [8, 48], day int64 [8] (the day indices).  Plain pickle and numpy only.
"""
import os
import pickle
import sys

import numpy as np

T = 24


def main(src):
    with open(os.path.join(src, "demand.pickle"), "rb") as f:
        load = np.asarray(pickle.load(f)["value"], dtype=np.float64)
    with open(os.path.join(src, "price.pickle"), "rb") as f:
        price = np.asarray(pickle.load(f)["SYS"], dtype=np.float64)
    days = min(len(load) // T, len(price) // T - 1)              # (a day needs the 24 hours after it for the look-ahead)
    lowest = min(int(np.argmin(price[:days * T])) // T, days - 1)
    pick = sorted(set(np.linspace(0, days - 1, 7).astype(int).tolist()) - {lowest}) + [lowest]
    spare = (d for d in range(days) if d not in pick)
    while len(pick) < 8:
        pick.append(next(spare))
    pick = np.array(sorted(pick), dtype=np.int64)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "evopf_days.npz")
    np.savez(out, load=np.stack([load[d * T:d * T + T] for d in pick]),
             price=np.stack([price[d * T:d * T + 2 * T] for d in pick]), day=pick)
    print("%s: days %s, lowest price %.2f" % (out, pick.tolist(), price[:days * T].min()))


if __name__ == "__main__":
    main(sys.argv[1])

"""CPU: Order::validate() of the host mirror (src/order_types.cpp:66-120) through the stand-alone
program tests/publish/test_order_validate: a hand table with one order per message plus STOP_LIMIT
with both prices bad, GTD without expiry, NaN and -0.0 quantities, lower-case `buy` and an
all-defaults order.  The expected texts are literal (publish_lib.hand_table); no device is used."""
import subprocess

import publish_lib as P

ALL_DEFAULTS = ["Order ID is required", "Base token is required", "Quote token is required",
                "Side must be 'BUY' or 'SELL'", "Quantity must be positive",
                "Limit price must be positive for LIMIT orders"]


def test_validate_hand_table(tmp_path):
    b, texts = P.hand_table()
    assert {t[0] for t in texts if len(t) == 1} >= {
        "Order ID is required", "Base token is required", "Quote token is required", "Side must be 'BUY' or 'SELL'",
        "Quantity must be positive", "Invalid order type: ICEBERG", "Limit price must be positive for LIMIT orders",
        "Stop price must be positive for STOP orders", "Stop price must be positive for STOP_LIMIT orders",
        "Limit price must be positive for STOP_LIMIT orders", "Invalid time in force: GTX",
        "Expiry timestamp required for GTD orders"}
    assert ["Stop price must be positive for STOP_LIMIT orders",
            "Limit price must be positive for STOP_LIMIT orders"] in texts
    src, dst = str(tmp_path / "orders.bin"), str(tmp_path / "errors.bin")
    P.write_orders(src, b, b"orders")
    r = subprocess.run([P.binary("test_order_validate"), src, dst], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "order validate: ok" in r.stdout, r.stdout + r.stderr
    out = P.Parse(dst)
    got = [[out.string().decode() for _ in range(out.u32())] for _ in range(b.n + 1)]
    assert out.done()
    assert got[0] == ALL_DEFAULTS  # a default-constructed Order (the program checks its member defaults too)
    for i, t in enumerate(texts):
        assert got[i + 1] == t, (i, got[i + 1], t)
    # the Python restatement the GPU tests use agrees with the mirror on every row
    for i, m in enumerate(b.masks()):
        assert [k for k in range(12) if int(m) >> k & 1] == \
               [next(k for k in range(12) if e.startswith(P.MESSAGES[k])) for e in got[i + 1]]

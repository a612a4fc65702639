/*! Expressions and statements: literals of every form, closures, loops with labels, patterns, `?` and turbofish.
 /* block comments nest */ and this line is still inside the outer one. */
use std::convert::TryFrom;
use std::error::Error;

/** A literal of each kind the lexer has to tell apart. */
pub fn literals() -> (u8, char, char, char, &'static str, &'static [u8], f64, u64, i128) {
    let byte = b'\'';
    let quote = '\'';
    let backslash = '\\';
    let unicode = '\u{1F600}';
    let raw = r#"a "raw" string with // no comment and /* no comment */"#;
    let bytes: &'static [u8] = br##"bytes "#" inside"##;
    let escaped = "tab\t quote\" newline\n brace { bracket [ paren (";
    let float = 1.5e-3 + 2.0_f64 + 3f64 + 0.25;
    let hex = 0xFFFF_FFFFu64 + 0o17 + 0b1010_1010 + 1_000;
    let big = -1_000_000_000_000_000_000_000i128;
    let _ = (escaped, b"byte string", c"c string", 'a'..='z', 1u8 as char);
    (byte, quote, backslash, unicode, raw, bytes, float, hex, big)
}

pub fn control(values: &[i64]) -> Result<i64, Box<dyn Error + Send + Sync + 'static>> {
    let mut total = 0i64;
    'outer: for (i, &v) in values.iter().enumerate() {
        let mut k = v;
        while k > 0 {
            if k % 7 == 0 {
                continue 'outer;
            }
            k /= 2;
        }
        total += match v {
            i64::MIN..=-1 => -v,
            0 => 0,
            1 | 2 | 3 => v * 2,
            x if x % 2 == 0 => x / 2,
            _ => i as i64,
        };
    }
    let n = loop {
        break 42;
    };
    let Some(first) = values.first() else {
        return Err("empty".into());
    };
    let parsed = "17".parse::<i64>()?;
    let small = u8::try_from(parsed)?;
    if let [a, b, rest @ ..] = values {
        total += a + b + rest.len() as i64;
    } else if values.is_empty() {
        total = 0;
    } else {
        total -= 1;
    }
    Ok(total + n + first + small as i64)
}

pub fn closures() -> Vec<u32> {
    let offset = 3;
    let add = |x: u32| -> u32 { x + offset };
    let twice = move |x| add(add(x));
    let boxed: Box<dyn Fn(u32) -> u32 + Send> = Box::new(|x| x << 1);
    let mut out: Vec<u32> = (0..8u32).map(twice).filter(|&x| x % 2 == 1).collect();
    out.extend([1, 2, 3].iter().map(|x| boxed(*x)));
    out.sort_unstable_by(|a, b| b.cmp(a));
    out.retain(|x| *x != 0);
    let _nested = vec![vec![0u8; 4]; 2];
    let _tuple = ((1, 2), [3, 4], (5,));
    let _range = &out[1..out.len() - 1];
    let _ref = &mut out[..];
    out
}

pub fn generic<T, F>(items: &[T], f: F) -> Option<T>
where
    T: Clone + PartialOrd,
    F: Fn(&T) -> bool,
{
    let mut best: Option<T> = None;
    for item in items.iter().filter(|x| f(x)) {
        best = match best {
            Some(b) if b >= *item => Some(b),
            _ => Some(item.clone()),
        };
    }
    best
}

pub fn unsafe_block(v: &mut [u32]) -> u32 {
    let p = v.as_mut_ptr();
    unsafe {
        *p.add(1) = 7;
        std::ptr::read(p.add(1))
    }
}

struct Guard<'a> {
    log: &'a mut Vec<&'static str>,
}

impl Drop for Guard<'_> {
    fn drop(&mut self) {
        self.log.push("dropped");
    }
}

pub fn lifetimes<'a, 'b: 'a>(x: &'a str, y: &'b str) -> &'a str {
    let mut log = Vec::new();
    {
        let _g = Guard { log: &mut log };
    }
    if x.len() > y.len() { x } else { y }
}
